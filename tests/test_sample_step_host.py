"""CPU tests around cs_sample_step: the state machine's restatement on scripted draws, the
seed rule against runtime.draw_seed, the Best-of-N ``generation`` key, and the ABI text."""
import os
import re
from importlib import import_module

import pytest

from conftest import REPO, PKG_DIR
from sample_step_ref import StepState, as_i64, seed_of

PAD = 9
# the restatement below describes an entry point of the library: no entry point, no tests
assert "cs_sample_step" in import_module(PKG_DIR + "._lib").EXPORTED


def scripted(rows):
    """draw(t) returning column t of per-stream id scripts; the log-prob is -(id + t/10)."""
    def draw(t):
        ids = [r[t] if t < len(r) else 1 for r in rows]
        return ids, [-(i + t / 10.0) for i in ids]
    return draw


def run(rows, max_tokens, stop=(5,), done=None, steps=None):
    st = StepState(len(rows), max_tokens, PAD, stop_ids=stop, done=done)
    trace = []
    for t in range(max_tokens if steps is None else steps):
        st.step(t, scripted(rows))
        trace.append((list(st.done), list(st.out_len), list(st.next_tok), st.n_alive))
    return st, trace


def test_stop_at_step_zero_appends_nothing():
    st, trace = run([[5, 3, 3]], 4)
    assert st.sequences() == [[]]
    assert trace[0] == ([1], [0], [PAD], 0)
    assert trace[-1] == ([1], [0], [PAD], 0)
    assert st.out_tokens[0] == [-7] * 4 and st.out_lp[0] == [-777.0] * 4


def test_stop_midway_keeps_the_tokens_before_it():
    st, trace = run([[3, 4, 5, 6, 6], [2, 2, 2, 2, 2]], 5)
    assert st.sequences() == [[3, 4], [2, 2, 2, 2, 2]]
    assert [tr[2] for tr in trace] == [[3, 2], [4, 2], [PAD, 2], [PAD, 2], [PAD, PAD]]
    assert [tr[3] for tr in trace] == [2, 2, 1, 1, 0]
    assert st.out_tokens[0][2:] == [-7] * 3          # the stop id is not appended
    assert st.out_lp[0][:2] == [-3.0, -4.1]


def test_no_drawable_logit_ends_the_stream():
    st, trace = run([[3, -1, 3]], 4)
    assert st.sequences() == [[3]]
    assert trace[1] == ([1], [1], [PAD], 0)


def test_max_tokens_one():
    st, trace = run([[3], [5]], 1)
    assert st.sequences() == [[3], []]
    assert trace == [([1, 1], [1, 0], [PAD, PAD], 0)]


def test_reaching_max_tokens_exactly():
    st, trace = run([[1, 2, 3]], 3)
    assert st.sequences() == [[1, 2, 3]]
    assert [tr[0] for tr in trace] == [[0], [0], [1]]
    assert [tr[2] for tr in trace] == [[1], [2], [PAD]]      # the last token is never fed back
    assert [tr[3] for tr in trace] == [1, 1, 0]


def test_stream_that_starts_done_is_untouched():
    st, trace = run([[1, 2, 3], [4, 4, 4]], 3, done=[1, 0])
    assert st.sequences() == [[], [4, 4, 4]]
    assert st.out_tokens[0] == [-7] * 3 and st.out_len[0] == 0
    assert [tr[2] for tr in trace] == [[PAD, 4], [PAD, 4], [PAD, PAD]]
    assert [tr[3] for tr in trace] == [1, 1, 0]


def test_stop_ids_outside_the_script_change_nothing():
    st, _ = run([[1, 2, 3]], 3, stop=(1000, -3))
    assert st.sequences() == [[1, 2, 3]]


@pytest.fixture(scope="module")
def runtime():
    return import_module(PKG_DIR + ".runtime")


@pytest.mark.parametrize("base", [0, 1, 1 << 63, (1 << 64) - 1, ((1 << 64) // 1000003) + 12345])
def test_seed_rule_is_runtime_draw_seed(runtime, base):
    for t in (0, 1, 7, 149, 4095):
        want = runtime.draw_seed(base, t)
        assert seed_of(base, t) == want
        assert 0 <= want < (1 << 64)
        # the int64 bit pattern torch stores, and back
        i = runtime.to_i64(want)
        assert -(1 << 63) <= i < (1 << 63) and i % (1 << 64) == want
        assert as_i64(want) == i
        # the kernel multiplies the stored uint64 word: starting from the int64 pattern of
        # the base gives the same seed
        assert seed_of(runtime.to_i64(base) % (1 << 64), t) == want
    wraps = ((1 << 64) // 1000003) + 12345
    assert wraps * 1000003 >= (1 << 64)      # this base does wrap


def test_generation_key_is_validated_before_any_engine(runtime, monkeypatch):
    bon = import_module(PKG_DIR + ".methods.best_of_n")

    def no_engine(*a, **k):
        raise AssertionError("the engine registry was touched")

    monkeypatch.setattr(runtime, "get_engine", no_engine)
    with pytest.raises(ValueError, match="generation"):
        bon.BestOfNGenerator("test/none", {"generation": "nonsense"})
    assert bon.BestOfNGenerator("test/none", {}).generation == "host"
    assert bon.BestOfNGenerator("test/none", {"generation": "device"}).generation == "device"


def _prototype(text, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_and_binding_agree():
    header = open(os.path.join(REPO, "include", "consensus_scoring.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib_src = open(os.path.join(REPO, PKG_DIR, "_lib.py")).read()
    for name in ("cs_sample_step_workspace_size", "cs_sample_step"):
        args = _prototype(header, name)
        assert f'"{name}"' in lib_src, f"{name} missing from _lib.EXPORTED"
        m = re.search(r"L\." + name + r"\.argtypes\s*=\s*\[(.*?)\]", lib_src, flags=re.S)
        assert m, f"{name} has no argtypes"
        bound = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert len(bound) == len(args), (name, len(bound), len(args))
        # pointers bind as void pointers, everything else does not
        for b, a in zip(bound, args):
            assert (b == "vp") == ("*" in a or a.startswith("cs_stream_t")), (name, b, a)
    assert len(_prototype(header, "cs_sample_step")) == 25
    assert _prototype(header, "cs_sample_step_workspace_size") == ["int64_t S", "int64_t vocab"]
