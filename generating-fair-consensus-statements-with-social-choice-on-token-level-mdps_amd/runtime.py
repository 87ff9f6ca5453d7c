"""Model-identifier -> scoring engine registry, and seeded generation on the engine.

The reference resolves a model identifier (e.g. "meta-llama/Meta-Llama-3.1-8B-Instruct-Turbo")
to a remote endpoint through the module-global Together ``client`` (src/utils.py:69-74).
Here the identifier resolves to a local ``ScoringEngine`` on the current HIP device:
  * one registered explicitly (``register_engine``; tests register the parity fixture
    model this way);
  * a local Hugging Face checkpoint directory (config.json + *.safetensors +
    tokenizer.json): the identifier itself when it is a directory, or
    ``$CS_MODEL_ROOT/<identifier>`` (``register_model_dir`` maps an id to a directory);
  * ``random:<preset>`` (e.g. ``random:llama-3.1-8b``): an architecture-exact,
    random-initialised bf16 model with a full-vocabulary synthetic tokenizer — for
    throughput benchmarks only, the statements it produces mean nothing.
An identifier ending in ``@fp8`` resolves as the identifier without the suffix (a checkpoint
directory or ``random:<preset>``), and the engine built for it is quantised once
(``Model.quantize_fp8``: FP8 e4m3 copies of the projection weights for the decode-step GEMMs,
the bf16 weights rounded onto the same grid) and cached under the full identifier; the
identifier without the suffix keeps its own, unrounded engine.
A real model id with none of these raises: random weights are never substituted
silently (set CS_ALLOW_RANDOM_INIT=1 to get the random-init model with a warning).

Concurrency: the reference runs generators in threads against one process
(src/experiment.py:283-322).  Everything that launches work on a device takes
``device_lock(device)`` (re-entrant), so forward passes and the kernels' shared
workspaces are used by one thread at a time per device.

Seed semantics of the local samplers (the replacement for the remote API's
``seed`` argument) are defined here once and restated by the test fake client:
  * a one-token draw with seed s uses the counter-based Gumbel noise g(s, v)
    (cs_vocab_sample);
  * token t of a multi-token generation with seed s uses seed ``draw_seed(s, t)``.
"""
from __future__ import annotations

import collections
import logging
import os
import re
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .engine import BeamState, ScoringEngine
from .model import Model, preset
from .tokenizer import CharTokenizer

_M64 = (1 << 64) - 1
_lock = threading.RLock()
_ENGINES: Dict[str, Tuple[ScoringEngine, CharTokenizer]] = {}
_MODEL_DIRS: Dict[str, str] = {}
_DEVICE_LOCKS: Dict[str, threading.RLock] = {}
_LOADING: Dict[str, threading.Lock] = {}
logger = logging.getLogger(__name__)

_NAME_TO_PRESET = [
    (r"3\.3-70b|llama-3\.3-70b|70b", "llama-3.3-70b"),
    (r"3\.1-8b|llama-3\.1-8b|8b", "llama-3.1-8b"),
    (r"3\.2-1b|1b", "llama-3.2-1b"),
    (r"gemma-2-9b|gemma", "gemma-2-9b"),
    (r"tiny-gemma", "tiny-gemma"),
    (r"tiny", "tiny-llama"),
]


def draw_seed(seed: int, t: int) -> int:
    """Seed of token t of a seeded multi-token generation."""
    return (int(seed) * 1000003 + int(t)) & _M64


def to_i64(seed: int) -> int:
    """uint64 seed -> the int64 bit pattern torch stores."""
    seed &= _M64
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def fresh_seed() -> int:
    return int.from_bytes(os.urandom(8), "little")


def device_lock(device) -> threading.RLock:
    """The re-entrant lock serialising work on one device (forward passes, workspaces)."""
    key = str(torch.device(device))
    with _lock:
        lk = _DEVICE_LOCKS.get(key)
        if lk is None:
            lk = _DEVICE_LOCKS[key] = threading.RLock()
        return lk


def serialized(attr: str = "model_identifier"):
    """Method decorator: run under the device lock of ``getattr(self, attr)``'s engine
    (the reference's runner calls generators from threads, src/experiment.py:283-322)."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrap(self, *a, **k):
            eng, _ = get_engine(getattr(self, attr))
            with device_lock(eng.device):
                return fn(self, *a, **k)
        return wrap
    return deco


def register_engine(model_identifier: str, engine: ScoringEngine, tokenizer: CharTokenizer) -> None:
    with _lock:
        _ENGINES[model_identifier] = (engine, tokenizer)


def register_model_dir(model_identifier: str, path: str) -> None:
    """Serve ``model_identifier`` from a local checkpoint directory (loaded on first use)."""
    with _lock:
        _MODEL_DIRS[model_identifier] = path


def random_engine(preset_name: str, device=None, dtype=torch.bfloat16, seed: int = 0,
                  tokenizer_dir: Optional[str] = None, **engine_kw):
    """Architecture-exact random-init model + a full-vocabulary tokenizer: the
    character tokenizer, or the BPE of ``tokenizer_dir`` (tokenizer.json; ids past its
    table are synthetic single characters) for realistic prompt token counts."""
    cfg = preset(preset_name)
    dev = torch.device(device) if device is not None else \
        torch.device("cuda", torch.cuda.current_device())
    model = Model(cfg, dev, dtype, seed=seed)
    fam = "gemma2" if cfg.family == "gemma2" else "llama3"
    if tokenizer_dir:
        from .tokenizer import BPETokenizer
        # the fixture's chat template is Llama-3's: other families use their own layout
        tok = BPETokenizer(tokenizer_dir, fam, vocab_size=cfg.vocab, use_config=fam == "llama3")
    else:
        tok = CharTokenizer(fam, vocab_size=cfg.vocab)
    return ScoringEngine(model, **engine_kw), tok


def clear_engines() -> None:
    with _lock:
        _ENGINES.clear()


# --- text encoders (the embedding model of the evaluator) ------------------------------
_ENCODERS: Dict[str, tuple] = {}


def register_encoder(model_identifier: str, encoder, tokenizer) -> None:
    """Serve ``model_identifier`` (e.g. "BAAI/bge-large-en-v1.5") from this TextEncoder and its
    tokenizer (``encode_many(texts) -> id lists``, framed and truncated)."""
    with _lock:
        _ENCODERS[model_identifier] = (encoder, tokenizer)


def clear_encoders() -> None:
    with _lock:
        _ENCODERS.clear()


def random_encoder(preset_name: str, device=None, seed: int = 0):
    """Architecture-exact random-init bf16 encoder + a stand-in tokenizer (benchmarks only)."""
    from .encoder import TextEncoder, preset as enc_preset
    from .tokenizer import RandomIdTokenizer

    cfg = enc_preset(preset_name)
    dev = torch.device(device) if device is not None else \
        torch.device("cuda", torch.cuda.current_device())
    return TextEncoder(cfg, dev, seed=seed), RandomIdTokenizer(cfg.vocab, cfg.n_pos)


def get_encoder(model_identifier: str):
    """(TextEncoder, tokenizer) serving ``model_identifier``, resolved in get_engine's order: one
    registered (``register_encoder``), a local BertModel checkpoint directory (the id itself,
    ``register_model_dir`` or ``$CS_MODEL_ROOT/<id>``), ``random:<preset>`` (e.g.
    ``random:bge-large-en-v1.5``).  Anything else raises CSError: no weights are made up."""
    with _lock:
        if model_identifier in _ENCODERS:
            return _ENCODERS[model_identifier]
        if not torch.cuda.is_available():
            raise ops.CSError("no HIP device: the text encoder has no CPU path")
        ld = _LOADING.setdefault("encoder:" + model_identifier, threading.Lock())
    with ld:
        with _lock:
            if model_identifier in _ENCODERS:
                return _ENCODERS[model_identifier]
            path = _model_dir(model_identifier)
        if path is not None:
            from .checkpoint import load_encoder
            ent = load_encoder(path)
        elif model_identifier.startswith("random:"):
            ent = random_encoder(model_identifier.split(":", 1)[1])
        else:
            raise ops.CSError(
                f"no weights for embedding model {model_identifier!r}: register an encoder "
                "(runtime.register_encoder), give a local BertModel checkpoint directory "
                "(config.json, *.safetensors, tokenizer.json) as the id, via "
                "runtime.register_model_dir or under $CS_MODEL_ROOT, or use 'random:<preset>'")
        with _lock:
            _ENCODERS[model_identifier] = ent
        return ent


def resolve_preset(model_identifier: str) -> str:
    name = model_identifier.lower()
    for pat, pre in _NAME_TO_PRESET[::-1] if name.startswith("tiny") else _NAME_TO_PRESET:
        if re.search(pat, name):
            return pre
    raise ValueError(f"no local architecture known for model identifier {model_identifier!r}")


def _model_dir(model_identifier: str) -> Optional[str]:
    if model_identifier in _MODEL_DIRS:
        return _MODEL_DIRS[model_identifier]
    if os.path.isdir(model_identifier) and os.path.exists(os.path.join(model_identifier, "config.json")):
        return model_identifier
    root = os.environ.get("CS_MODEL_ROOT")
    if root:
        cand = os.path.join(root, model_identifier)
        if os.path.exists(os.path.join(cand, "config.json")):
            return cand
    return None


# --- GEMM solution selection -------------------------------------------------------
GEMM_TUNING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gemm_mi355x.csv")
_gemm_tuning: Optional[str] = None
_gemm_tuning_tried = False


def use_gemm_tuning(path: Optional[str] = None) -> Optional[str]:
    """Pick each forward GEMM's hipBLASLt solution from a committed PyTorch TunableOp
    results file (measured on MI355X by tools/tune_gemms.py) instead of the library
    heuristic — read only, no tuning at run time; shapes not in the file keep the heuristic.
    Returns the file in use (None: not used).

    TunableOp is process-wide (every later matmul of the process, bf16 rounding included,
    follows the file), so this is OPT-IN: call it (bench.py does), or set CS_GEMM_TUNING=1
    (the committed file) / CS_GEMM_TUNING=<file> to have ``get_engine`` call it.  An
    explicit TunableOp session (PYTORCH_TUNABLEOP_ENABLED in the environment, e.g. while
    tuning) is left alone; CS_GEMM_TUNING=0 disables.  Nothing is written back on exit."""
    global _gemm_tuning, _gemm_tuning_tried
    with _lock:
        if _gemm_tuning_tried and path is None:
            return _gemm_tuning
        _gemm_tuning_tried = True
        env = os.environ.get("CS_GEMM_TUNING")
        if env == "0" or "PYTORCH_TUNABLEOP_ENABLED" in os.environ or not torch.cuda.is_available():
            return None
        if env == "1":
            env = None
        path = path or env or GEMM_TUNING
        if not os.path.exists(path):
            return None
        import tempfile

        import torch.cuda.tunable as tunable
        try:
            tunable.enable(True)
            tunable.tuning_enable(False)
            tunable.record_untuned_enable(False)
            # the committed file is read only: no write-back at exit (and none to it)
            if hasattr(tunable, "write_file_on_exit"):
                tunable.write_file_on_exit(False)
            tunable.set_filename(os.path.join(tempfile.gettempdir(), f"cs_tunableop_{os.getpid()}.csv"))
            ok = tunable.read_file(path)
        except Exception as e:   # no usable device / TunableOp unavailable: library heuristic
            logger.warning("GEMM tuning file %s not loaded: %s", path, e)
            return None
        if not ok:
            logger.warning("GEMM tuning file %s not usable here (versions differ?)", path)
            tunable.enable(False)
            return None
        _gemm_tuning = path
        logger.info("GEMM solutions from %s (PyTorch TunableOp, process-wide, read only)", path)
        return path


FP8_SUFFIX = "@fp8"


def split_fp8_id(model_identifier: str) -> Tuple[str, bool]:
    """(the identifier without a trailing ``@fp8``, whether it had one)."""
    if model_identifier.endswith(FP8_SUFFIX) and len(model_identifier) > len(FP8_SUFFIX):
        return model_identifier[:-len(FP8_SUFFIX)], True
    return model_identifier, False


def get_engine(model_identifier: str) -> Tuple[ScoringEngine, CharTokenizer]:
    """The engine serving ``model_identifier``; loaded on first use.  A load (minutes for a
    70B checkpoint) holds only that identifier's loading lock, not the registry lock, so
    threads working on already-loaded engines are not stalled by it."""
    with _lock:
        if model_identifier in _ENGINES:
            return _ENGINES[model_identifier]
        if not torch.cuda.is_available():
            raise ops.CSError("no HIP device: the scoring engine has no CPU path")
        ld = _LOADING.setdefault(model_identifier, threading.Lock())
    with ld:
        with _lock:
            if model_identifier in _ENGINES:     # loaded by another thread meanwhile
                return _ENGINES[model_identifier]
            base, fp8 = split_fp8_id(model_identifier)
            path = _model_dir(base)
            loadable = path is not None or base.startswith("random:") or \
                os.environ.get("CS_ALLOW_RANDOM_INIT") == "1"
            if fp8 and not loadable and base in _ENGINES:
                raise ops.CSError(
                    f"model {base!r} is a registered engine object: quantise a copy of it "
                    f"(engine.model.quantize_fp8()) and register that as {model_identifier!r}")
        # an @fp8 id builds its own engine: the one cached under the plain id stays unrounded
        ent = _load_engine(base, path)
        if fp8:
            with device_lock(ent[0].model.device):
                ent[0].model.quantize_fp8()      # (CSError unless bf16 on a HIP device)
        if os.environ.get("CS_GEMM_TUNING", "0") != "0":
            use_gemm_tuning()
        with _lock:
            _ENGINES[model_identifier] = ent
        return ent


def _load_engine(model_identifier: str, path: Optional[str]):
    """Construct the engine of an identifier (no registry lock held)."""
    if path is not None:
        from .checkpoint import load_engine
        ent = load_engine(path)
    elif model_identifier.startswith("random:"):
        ent = random_engine(model_identifier.split(":", 1)[1])
    elif os.environ.get("CS_ALLOW_RANDOM_INIT") == "1":
        name = resolve_preset(model_identifier)
        logger.warning("model %r: no checkpoint found; using RANDOM-INIT %s weights "
                       "(CS_ALLOW_RANDOM_INIT=1) -- statements will be meaningless",
                       model_identifier, name)
        ent = random_engine(name)
    else:
        raise ops.CSError(
            f"no weights for model {model_identifier!r}: register an engine "
            "(runtime.register_engine), give a local checkpoint directory (config.json, "
            "*.safetensors, tokenizer.json) as the id, via runtime.register_model_dir or "
            "under $CS_MODEL_ROOT, or use 'random:<preset>' for an architecture-exact "
            "random-init benchmark model")
    return ent


# --- logit bias -------------------------------------------------------------------
def bias_token_ids(tok: CharTokenizer, strings: Optional[Sequence[str]]) -> List[int]:
    """Ids the reference biases for ``strings``.

    Semantics of get_token_ids (src/utils.py:466-525: token map of the chat-rendered
    single-user-message prompt) followed by the containment filter
    ``{t: id for t, id in map.items() if s in t}`` (src/utils.py:124-136,
    src/methods/beam_search.py:240-251).
    """
    if not strings:
        return []
    if isinstance(strings, str):
        strings = [strings]
    out: List[int] = []
    for s in strings:
        ids, _ = tok.render_chat(None, s)
        tmap = {}
        for i in ids:
            tmap[tok.token_str(i)] = i
        for t, i in tmap.items():
            if s in t and i not in out:
                out.append(i)
    return out


def apply_bias(logits: torch.Tensor, ids: Sequence[int], value: float) -> torch.Tensor:
    if ids:
        idx = torch.as_tensor(list(ids), dtype=torch.long, device=logits.device)
        logits[:, idx] = logits[:, idx] + value
    return logits


# --- stop strings -------------------------------------------------------------------
STOP_TAIL = 31      # bytes of decoded text kept between steps (cs_sample_step_ex's window)
_BARRIER = b"\xff"  # never in UTF-8 text: stands for a token whose text the table lacks


def early_stop_strings(stop_strings: Optional[Sequence[str]]) -> List[bytes]:
    """The stop strings a generation loop may end a stream on BEFORE the caller cuts the
    text (utils.generate_text: text[:text.find(term)] for each terminator in turn), without
    changing what that cut returns: ASCII strings of 1 to 32 bytes, at most 8 of them (a
    byte match in the token bytes is then a match in the decoded text at the same place).
    None are used if two different strings can overlap in a text with the second ending
    later (one inside the other, or a suffix of one opening the other): the cut could then
    find in the longer text an occurrence that the stopped text no longer holds."""
    if isinstance(stop_strings, str):
        stop_strings = [stop_strings]
    terms = [t for t in dict.fromkeys(stop_strings or ()) if t]
    for a in terms:
        for b in terms:
            if a is not b and (b in a or any(a.startswith(b[k:]) for k in range(1, len(b)))):
                return []
    ok = [t.encode("ascii") for t in terms if t.isascii() and len(t) <= ops.MAX_STOP_LEN]
    return ok[:ops.MAX_STOP_SEQ]


def stop_token_table(tok, vocab: int) -> Optional[List[bytes]]:
    """Token id -> bytes for ids [0, vocab) from tok.token_bytes() (None if the tokenizer has
    no exact table).  A token without bytes there (a special token, an id past the
    tokenizer's vocabulary) gets one byte no stop string holds, so no match spans it."""
    tb = tok.token_bytes() if hasattr(tok, "token_bytes") else None
    if tb is None:
        return None
    key = (id(tb), int(vocab))
    cached = getattr(tok, "_stop_table", None)
    if cached is None or cached[0] != key:
        data, off = tb
        n = len(off) - 1
        table = [data[off[i]:off[i + 1]] or _BARRIER if i < n else _BARRIER for i in range(vocab)]
        cached = tok._stop_table = (key, table, {})
    return cached[1]


def _stop_table_device(tok, vocab: int, dev):
    """(tok_bytes uint8, tok_off int32 [vocab + 1]) of stop_token_table on ``dev``, built
    once per tokenizer and device."""
    table = stop_token_table(tok, vocab)
    if table is None:
        return None
    per_dev = tok._stop_table[2]
    if str(dev) not in per_dev:
        import numpy as np
        off = np.zeros(vocab + 1, dtype=np.int32)
        np.cumsum([len(b) for b in table], out=off[1:])
        data = np.frombuffer(b"".join(table) + b"\0", dtype=np.uint8).copy()
        per_dev[str(dev)] = (torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev))
    return per_dev[str(dev)]


def stop_window_push(tail: bytes, piece: bytes, stops: Sequence[bytes]):
    """cs_sample_step_ex's window rule on the host: (hit, new tail) after a token with bytes
    ``piece``; hit if a stop string occurs in tail + piece ending inside piece."""
    if not piece:
        return False, tail
    w = tail + piece
    hit = any(w.find(s, max(0, len(tail) + 1 - len(s))) != -1 for s in stops)
    return hit, w[-STOP_TAIL:]


def _ragged_i32(lists, dev):
    """(ids, offsets) int32 device tensors of per-row id lists (ops' seen_ids / seen_off)."""
    off = [0]
    for r in lists:
        off.append(off[-1] + len(r))
    flat = [int(i) for r in lists for i in r] + [0]          # never an empty allocation
    return (torch.tensor(flat, dtype=torch.int32, device=dev)[:off[-1]],
            torch.tensor(off, dtype=torch.int32, device=dev))


# --- constrained sampling -----------------------------------------------------------
class Constraint:
    """What compile_constraint returns: an automaton over the text's bytes (one table, one
    start state per pattern), the stop ids it was built for and the tokenizer's byte table;
    the device copies (token masks, transitions, byte table) are built on first use, once per
    device and vocabulary size."""

    def __init__(self, dfa, starts: List[int], stop_ids: Tuple[int, ...], tok_bytes, tok_off,
                 shared: Optional[dict] = None) -> None:
        self.dfa, self.starts, self.stop_ids = dfa, list(starts), tuple(stop_ids)
        self._bytes, self._off = tok_bytes, tok_off
        self._dev = {} if shared is None else shared

    def select(self, k: int) -> "Constraint":
        """The constraint of pattern k alone (the same tables, one start state)."""
        return Constraint(self.dfa, [self.starts[k]], self.stop_ids, self._bytes, self._off,
                          self._dev)

    def token_bytes(self, v: int) -> bytes:
        """Token v's bytes (none for a special token or an id past the table)."""
        return self._bytes[self._off[v]:self._off[v + 1]] if 0 <= v < len(self._off) - 1 else b""

    def advance(self, state: int, v: int) -> int:
        """The state after token v (the walk of cs_sample_step_dfa)."""
        return self.dfa.walk(state, self.token_bytes(v))

    def device(self, dev, vocab: int):
        """(masks, trans, tok_bytes, tok_off) on ``dev`` for a model of ``vocab`` ids; ids past
        the tokenizer's table have no bytes, so they are never drawable."""
        key = (str(dev), int(vocab))
        if key not in self._dev:
            import numpy as np
            n = len(self._off) - 1
            off = np.full(vocab + 1, self._off[min(n, vocab)], dtype=np.int32)
            off[:min(n, vocab) + 1] = self._off[:min(n, vocab) + 1]
            data = np.frombuffer(bytes(self._bytes) + b"\0", dtype=np.uint8).copy()
            tb, to = torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev)
            trans = torch.from_numpy(self.dfa.trans.copy()).to(dev)
            accept = torch.from_numpy(self.dfa.accept.astype(np.uint8)).to(dev)
            stop = [i for i in self.stop_ids if 0 <= i < vocab]
            stop_t = torch.tensor(stop, dtype=torch.int32, device=dev) if stop else None
            self._dev[key] = (ops.dfa_token_masks(trans, accept, tb, to, stop_t), trans, tb, to)
        return self._dev[key]


def _spec_dfa(spec):
    """(cache key, Dfa) of one constraint spec: a regex, a Dfa or {"type": "json_object"}."""
    from . import constrain
    if isinstance(spec, constrain.Dfa):
        return ("dfa", spec.key()), spec
    if isinstance(spec, str):
        return ("re", spec), constrain.compile_regex(spec)
    if isinstance(spec, dict):
        if spec.get("type") != "json_object" or set(spec) - {"type", "max_depth"}:
            raise ValueError(f"unsupported constraint {spec!r}: only "
                             '{"type": "json_object"} (with an optional "max_depth")')
        depth = int(spec.get("max_depth", 2))
        return ("json", depth), constrain.json_object(depth)
    raise TypeError(f"a constraint is a regex string, a Dfa or a dict, not {type(spec).__name__}")


_SPEC_CACHE = 32


def compile_constraint(tok, spec, stop_ids: Optional[Sequence[int]] = None) -> Constraint:
    """The sampling constraint of ``spec`` for tokenizer ``tok``: a regex string
    (constrain.compile_regex: full match), a constrain.Dfa, {"type": "json_object"} (one JSON
    object, constrain.json_object(2)), or a list of those, one per prompt of generate_streams
    (joined into one table by constrain.union).  ``stop_ids`` (default tok.eos_ids) are the
    ids that may end a stream, drawable in accepting states only; generate / generate_streams
    must be called with the same ones.

    Built once per (tokenizer, spec, stop ids).  The tokenizer's exact token_bytes() table is
    required (CharTokenizer and byte-level BPETokenizer have one): without it CSError, since a
    constraint that silently did nothing would be worse than none."""
    from . import constrain
    tb = tok.token_bytes() if hasattr(tok, "token_bytes") else None
    if tb is None:
        raise ops.CSError(f"compile_constraint: {type(tok).__name__} has no exact token_bytes() "
                          "table, so a token's effect on the pattern cannot be known")
    stop = tuple(int(i) for i in (tok.eos_ids if stop_ids is None else stop_ids))
    many = isinstance(spec, (list, tuple))
    keyed = [_spec_dfa(s) for s in (spec if many else [spec])]
    if not keyed:
        raise ValueError("compile_constraint: an empty list of patterns")
    key = (many, tuple(k for k, _ in keyed), tuple(sorted(set(stop))))
    cache = tok.__dict__.setdefault("_constraints", collections.OrderedDict())
    if key not in cache:
        if many:
            dfa, starts = constrain.union([d for _, d in keyed])
        else:
            dfa, starts = keyed[0][1], [keyed[0][1].start]
        cache[key] = Constraint(dfa, starts, stop, bytes(tb[0]), [int(o) for o in tb[1]])
        while len(cache) > _SPEC_CACHE:
            cache.popitem(last=False)
    return cache[key]


def _constraint_starts(constraint: Constraint, stop: Sequence[int], n_prompts: int) -> List[int]:
    """One start state per prompt, after checking that the masks were built for ``stop``."""
    if not isinstance(constraint, Constraint):
        raise TypeError("constraint must come from runtime.compile_constraint")
    if set(constraint.stop_ids) != set(int(i) for i in stop):
        raise ops.CSError("the constraint was compiled for other stop ids than this call uses: "
                          "pass the same stop_ids to compile_constraint")
    if len(constraint.starts) == 1:
        return constraint.starts * n_prompts
    if len(constraint.starts) != n_prompts:
        raise ValueError(f"{len(constraint.starts)} patterns for {n_prompts} prompts")
    return list(constraint.starts)


# --- seeded generation on the engine ------------------------------------------------
@torch.no_grad()
def generate(engine: ScoringEngine, tok: CharTokenizer, prefix_ids: Sequence[int],
             seeds: Sequence[Optional[int]], max_tokens: int, temperature: float = 1.0,
             bias_ids: Sequence[int] = (), bias_value: float = -1e6,
             stop_ids: Optional[Sequence[int]] = None, repetition_penalty: float = 1.0,
             stop_strings: Optional[Sequence[str]] = None,
             constraint: Optional[Constraint] = None) -> List[List[int]]:
    """Sample len(seeds) continuations of one prefix in a batch (token t of stream i
    drawn with seed draw_seed(seeds[i], t)); a stream stops after a stop token (not
    included) or max_tokens tokens.

    temperature 0 decodes greedily, repetition_penalty != 1 penalises the prompt's and the
    stream's own tokens (ops.vocab_sample_ex: the row transform of the device loop), and a
    stream also ends with the token that completes one of early_stop_strings(stop_strings)
    (included, so the caller's cut sees it).  With the defaults the draws are
    ops.vocab_sample's as before.

    ``constraint`` (compile_constraint, one pattern) holds every stream to its automaton:
    the state is kept here on the host and each draw is ops.vocab_sample_dfa's, so only
    tokens whose bytes keep the pattern alive are drawn, and a stop token only where the text
    matches.  A stream that no token can continue ends there; one that reaches max_tokens
    before the pattern is complete returns its prefix, which does not match."""
    n = len(seeds)
    seeds = [fresh_seed() if s is None else int(s) for s in seeds]
    stop = set(tok.eos_ids if stop_ids is None else stop_ids)
    out: List[List[int]] = [[] for _ in range(n)]
    if n == 0 or max_tokens <= 0:
        return out
    cache = engine.prefill([list(prefix_ids)])
    st = BeamState(engine, cache, n_prefix=1)
    alive = list(range(n))          # stream ids, in beam order
    dev = engine.device
    temperature, penalty = float(temperature), float(repetition_penalty)
    controls = temperature == 0.0 or penalty != 1.0 or constraint is not None
    stops = early_stop_strings(stop_strings)
    table = stop_token_table(tok, engine.model.cfg.vocab) if stops else None
    tails = [b""] * n
    dfa = {}
    if constraint is not None:
        states = _constraint_starts(constraint, stop, 1) * n
        dfa["masks"] = constraint.device(dev, engine.model.cfg.vocab)[0]
    bias_t = torch.tensor(list(bias_ids), dtype=torch.int32, device=dev) \
        if controls and len(bias_ids) else None
    prefix_ids = list(prefix_ids)
    for t in range(max_tokens):
        logits = st.next_logits(0).float() if st.n_beams == len(alive) else None
        if st.n_beams == 1 and len(alive) > 1:
            logits = engine.model.lm_head(st.next_hidden).float().expand(len(alive), -1).contiguous()
        sd = torch.tensor([[to_i64(draw_seed(seeds[i], t))] for i in alive], dtype=torch.int64,
                          device=dev)
        if controls:
            seen_ids, seen_off = _ragged_i32([prefix_ids + out[i] for i in alive], dev) \
                if penalty != 1.0 else (None, None)
            if constraint is not None:
                dfa["dfa_state"] = torch.tensor([states[i] for i in alive], dtype=torch.int32,
                                                device=dev)
            draw = ops.vocab_sample_ex if constraint is None else ops.vocab_sample_dfa
            ids, _ = draw(logits, sd, temperature=temperature, softcap=engine.softcap,
                          bias_ids=bias_t, bias_value=float(bias_value),
                          repetition_penalty=penalty, seen_ids=seen_ids, seen_off=seen_off, **dfa)
        else:
            logits = apply_bias(logits, bias_ids, bias_value)
            ids, _ = ops.vocab_sample(logits, sd, temperature=temperature, softcap=engine.softcap)
        ids = ids[:, 0].tolist()
        parent, toks, nxt = [], [], []
        for j, (i, v) in enumerate(zip(alive, ids)):
            if v in stop or v < 0:          # -1: the pattern allows no token here
                continue
            out[i].append(v)
            if constraint is not None:
                states[i] = constraint.advance(states[i], v)
            if table is not None:
                hit, tails[i] = stop_window_push(tails[i], table[v], stops)
                if hit:
                    continue
            if t + 1 < max_tokens:
                parent.append(0 if st.n_beams == 1 else j)
                toks.append(v)
                nxt.append(i)
        if not nxt:
            break
        st.advance(parent, toks)
        alive = nxt
    return out


def _seed_lists(seeds, n_prompts: int) -> List[List[int]]:
    """generate_streams' ``seeds``: one list for every prompt, or one list per prompt."""
    seeds = list(seeds)
    if seeds and all(isinstance(s, (list, tuple)) for s in seeds):
        if len(seeds) != n_prompts:
            raise ValueError(f"{len(seeds)} seed lists for {n_prompts} prompts")
        per = [list(s) for s in seeds]
    else:
        per = [list(seeds) for _ in range(n_prompts)]
    return [[fresh_seed() if s is None else int(s) for s in row] for row in per]


@torch.no_grad()
def generate_streams(engine: ScoringEngine, tok: CharTokenizer,
                     prefixes: Sequence[Sequence[int]], seeds, max_tokens: int,
                     temperature: float = 1.0, bias_ids: Sequence[int] = (),
                     bias_value: float = -1e6, stop_ids: Optional[Sequence[int]] = None,
                     poll_every: int = 8, return_logprobs: bool = False,
                     repetition_penalty: float = 1.0,
                     stop_strings: Optional[Sequence[str]] = None,
                     constraint: Optional[Constraint] = None):
    """Sample continuations of many prompts at once with the loop closed on the device:
    result[p][i] = the tokens of prompt p under seeds[p][i] (``seeds``: one list used for
    every prompt, or one list per prompt, of any lengths), drawn as ``generate`` draws
    them (token t with draw_seed(seed, t), a stop token ends the stream and is not
    included).  With ``return_logprobs`` the result is (tokens, log-probs), same nesting.

    One DecodeState holds every stream; a step is one graph replay whose last launches are
    the LM head and cs_sample_step, which appends the draw and writes the next step's input
    token on the device.  The host reads one word (the number of unfinished streams) every
    ``poll_every`` steps and downloads the tokens once at the end.  bf16 engines only: the
    stream decode is the bf16 path, and another dtype raises instead of changing numerics.

    temperature 0, repetition_penalty and stop_strings are ``generate``'s, applied inside the
    step (cs_sample_step_ex): each stream's prompt ids are its seen list, which the step
    extends by the tokens generated so far, and a stream ends with the token whose bytes
    complete one of early_stop_strings(stop_strings) -- where the tokenizer has an exact
    token_bytes() table; otherwise the streams run on to a stop token or max_tokens as
    before.  With the defaults the step is cs_sample_step.

    ``constraint`` (compile_constraint: one pattern for every prompt, or one per prompt) is
    ``generate``'s, with each stream's automaton state kept on the device and advanced inside
    the step (cs_sample_step_dfa), so the graph replays as before.  A stream cut at
    max_tokens returns a prefix that does not match yet."""
    from .engine import DecodeState
    P = len(prefixes)
    per = _seed_lists(seeds, P)
    B = max((len(r) for r in per), default=0)
    max_tokens = int(max_tokens)
    toks: List[List[List[int]]] = [[[] for _ in r] for r in per]
    lps: List[List[List[float]]] = [[[] for _ in r] for r in per]
    if P == 0 or B == 0 or max_tokens <= 0:
        return (toks, lps) if return_logprobs else toks
    m = engine.model
    if m.dtype != torch.bfloat16:
        raise ops.CSError(f"generate_streams needs a bf16 engine (this one is {m.dtype}): the "
                          "stream decode is the bf16 path; runtime.generate serves every dtype")
    if not m.fused_ok():
        raise ops.CSError(f"generate_streams: the stream kernels do not serve this model's heads "
                          f"(head_dim {m.cfg.head_dim}); runtime.generate does")
    stop = list(tok.eos_ids if stop_ids is None else stop_ids)
    dev = engine.device
    S = P * B
    with device_lock(dev):
        sp = engine.prefill_streams([list(p) for p in prefixes])
        ds = DecodeState(engine, sp, n_prefix=P, n_beams=B, max_steps=max(1, max_tokens - 1),
                         use_graphs=True)
        try:
            base = [to_i64(r[b]) if b < len(r) else 0 for r in per for b in range(B)]
            done0 = [0 if b < len(r) else 1 for r in per for b in range(B)]
            base_t = torch.tensor(base, dtype=torch.int64, device=dev)
            done = torch.tensor(done0, dtype=torch.int32, device=dev)
            out_len = torch.zeros(S, dtype=torch.int32, device=dev)
            out_tok = torch.zeros(S, max_tokens, dtype=torch.int32, device=dev)
            out_lp = torch.zeros(S, max_tokens, dtype=torch.float32, device=dev) \
                if return_logprobs else None
            n_alive = torch.zeros(1, dtype=torch.int32, device=dev)
            alive_h = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            bias_t = torch.tensor(list(bias_ids), dtype=torch.int32, device=dev) if bias_ids else None
            stop_t = torch.tensor(stop, dtype=torch.int32, device=dev) if stop else None
            pad_id = int(tok.eos_ids[0]) if getattr(tok, "eos_ids", None) else 0
            ws = ops.Workspace(zeroed=True)
            penalty = float(repetition_penalty)
            stops = early_stop_strings(stop_strings)
            tables = _stop_table_device(tok, m.cfg.vocab, dev) if stops else None
            if tables is None:
                stops = []
            ex = {}
            if float(temperature) == 0.0 or penalty != 1.0 or stops:
                ex = dict(repetition_penalty=penalty, stop_seqs=stops)
                if penalty != 1.0:
                    ex["seen_ids"], ex["seen_off"] = _ragged_i32(
                        [list(prefixes[p]) for p in range(P) for _ in range(B)], dev)
                if stops:
                    ex.update(tok_bytes=tables[0], tok_off=tables[1],
                              tail=torch.zeros(S, ops.MAX_STOP_LEN, dtype=torch.uint8, device=dev),
                              tail_len=torch.zeros(S, dtype=torch.int32, device=dev))
            if constraint is not None:
                starts = _constraint_starts(constraint, stop, P)
                masks, trans, tb, to = constraint.device(dev, m.cfg.vocab)
                ex.setdefault("repetition_penalty", penalty)
                # the constraint's byte table serves the stop strings too: a token without
                # bytes is never drawn under a constraint
                ex.update(masks=masks, trans=trans, tok_bytes=tb, tok_off=to,
                          dfa_state=torch.tensor([starts[p] for p in range(P) for _ in range(B)],
                                                 dtype=torch.int32, device=dev))
            step_op = ops.sample_step_dfa if constraint is not None else \
                ops.sample_step_ex if ex else ops.sample_step

            def post():
                logits = m.lm_head(ds.hidden)                      # [S, V]
                step_op(logits, base_t, ds.hist_base, done, out_len, out_tok, ds.tok,
                        n_alive, pad_id=pad_id, temperature=float(temperature),
                        softcap=engine.softcap, bias_ids=bias_t,
                        bias_value=float(bias_value), stop_ids=stop_t, out_lp=out_lp,
                        workspace=ws, **ex)

            post()                                 # token 0: every stream = its prompt
            every = max(1, int(poll_every))
            for a in range(max_tokens - 1):
                if a % every == 0:
                    alive_h.copy_(n_alive, non_blocking=True)
                    torch.cuda.current_stream().synchronize()
                    if int(alive_h[0]) == 0:
                        break
                ds.advance_device(post=post)
            lens_h = out_len.cpu().tolist()        # one download (synchronises)
            tok_h = out_tok.cpu().numpy()
            lp_h = out_lp.cpu().numpy() if return_logprobs else None
        finally:
            ds.release()
    for p, r in enumerate(per):
        for b in range(len(r)):
            s = p * B + b
            toks[p][b] = tok_h[s, :lens_h[s]].tolist()
            if return_logprobs:
                lps[p][b] = lp_h[s, :lens_h[s]].tolist()
    return (toks, lps) if return_logprobs else toks
