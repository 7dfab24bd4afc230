"""The kept[] bitmap of the span-granular tracker's loc[] through the kernel-logic harness (tests/emu), on the default build and on
the build with the structural checker (LM_EMU_CHECK: the bits are exactly the heads and the multiples of 64, loc[] is the item's leaf
wherever the bit is set).  Every case runs with LM_LOC_POISON unset and =1 (loc[] := 0 in front of the integrate stage): the results
are the oracle's bytes both times — no result depends on an entry whose bit is clear.  Where the plain merge model (_merge_ref)
models the document, its bytes are checked too.  The documents: tests/_loc_bitmap_docs.py."""
import ctypes

import pytest

import _emu, _loc_bitmap_docs as D, _oracle, _resident
from loro_amd._cabi import Context

_BINDINGS = {}


@pytest.fixture(scope="module", params=["default", "LM_EMU_CHECK"])
def binding(request):
    if request.param not in _BINDINGS:
        _BINDINGS[request.param] = _emu.binding() if request.param == "default" else _emu.variant(["LM_EMU_CHECK"])
    return _BINDINGS[request.param]


def _loc_stat(b, i):
    f = b.lib.lmemu_loc_stat
    f.restype, f.argtypes = ctypes.c_uint64, [ctypes.c_int]
    return f(i)


def _both(monkeypatch, run):
    """run() with LM_LOC_POISON unset and =1"""
    monkeypatch.delenv("LM_LOC_POISON", raising=False)
    plain = run()
    monkeypatch.setenv("LM_LOC_POISON", "1")
    poisoned = run()
    assert plain == poisoned
    return plain


def _merge(binding, docs, fr=None):
    with Context(binding) as c:
        return c.merge_batch(docs, fr)


def _check_group(binding, monkeypatch, group, model=True):
    docs = [d for d, _ in group]
    want = _oracle.merge_batch(docs)
    assert all(w[0] == 0 for w in want)
    if model:
        assert [D.model_result(reps) for _, reps in group] == want
    assert _both(monkeypatch, lambda: _merge(binding, docs)) == want


def test_window_edges(binding, monkeypatch):
    _loc_stat(binding, -1)
    _check_group(binding, monkeypatch, D.corpus()["edges"])
    _loc_stat(binding, -1)
    _check_group(binding, monkeypatch, D.corpus()["edge_sessions"])
    print("ts_loc_find calls of the sessions aimed at the window edges", _loc_stat(binding, 0))
    assert _loc_stat(binding, 0) >= 2 * 50   # (elements at the edges were looked up by id, in both runs)


def test_lookup_cut_lookup_in_one_window(binding, monkeypatch):
    c = D.corpus()
    monkeypatch.delenv("LM_LOC_POISON", raising=False)
    _loc_stat(binding, -1)
    _merge(binding, [d for d, _ in c["windows"]])
    calls, changed = _loc_stat(binding, 0), _loc_stat(binding, 1)
    print("ts_loc_find calls", calls, "lookups of a window whose bits changed since its previous lookup", changed)
    assert calls >= 50 and changed >= 10, (calls, changed)
    _check_group(binding, monkeypatch, c["windows"])
    _check_group(binding, monkeypatch, c["fuzz"])


def test_neighbours_twice_in_one_context(binding, monkeypatch):
    group = D.corpus()["neighbours"]
    docs = [d for d, _ in group]
    want = _oracle.merge_batch(docs)
    assert all(w[0] == 0 for w in want)
    assert [D.model_result(reps) for _, reps in group[:7]] == want[:7]
    order = [4, 8, 0, 6, 2, 7, 1, 5, 3]   # every slice moves

    def run():
        with Context(binding) as c:
            first = c.merge_batch(docs)
            second = c.merge_batch([docs[i] for i in order])
            third = c.merge_batch(docs)
        return first, second, third
    first, second, third = _both(monkeypatch, run)
    assert first == want and third == want and second == [want[i] for i in order]


def test_retry_launch_replays_from_cleared_bits(binding, monkeypatch):
    monkeypatch.setenv("LM_DIR_OPT_MAX", "4")
    group = D.corpus()["retry"] + D.corpus()["edges"][4:]
    docs = [d for d, _ in group]
    want = _oracle.merge_batch(docs)
    assert all(w[0] == 0 for w in want) and [D.model_result(reps) for _, reps in group] == want

    def run():
        with Context(binding) as c:
            got = c.merge_batch(docs)
            assert c.sizing()[3] >= 2, c.sizing()   # documents the retry launch replayed: the two "retry" sessions at least
        return got
    for memset in ("1", "0"):
        monkeypatch.setenv("LM_LOC_MEMSET", memset)
        assert _both(monkeypatch, run) == want


def test_resident_same_layout_and_renumbering(binding, monkeypatch):
    sessions = [D.resident_session()]
    want = _resident.oracle_sessions(sessions)
    assert all(w[0][0] == 0 for w in want)
    fresh = []

    def run():
        with Context(binding) as c:
            run0 = c.run

            def counting():
                run0()
                fresh.append(c.resident_fresh())
            c.run = counting
            return _resident.run_sessions(c, sessions)
    assert _both(monkeypatch, run) == want
    n = len(sessions[0])
    print("documents replayed from the empty version per run", fresh)
    assert fresh[0] == 1 and sum(fresh[1:n]) == 0, fresh   # every later run continues from the stored tracker (kept layout, then renumbered)


def test_mixed_batch(binding, monkeypatch):
    docs, fr = D.mixed_batch()
    want = _oracle.merge_batch(docs, frontiers=fr)
    assert all(w[0] == 0 for w in want)
    for auto in ("1", "0"):   # the kernels the batch's statistics pick, and the span-granular kernels whatever they say
        monkeypatch.setenv("LM_SPAN_AUTO", auto)
        assert _both(monkeypatch, lambda: _merge(binding, docs, fr)) == want
