"""GPU: the kept[] bitmap of the span-granular tracker's loc[] (lm_k_integrate_span.h sp_keep / ts_loc_find) — the documents of
tests/_loc_bitmap_docs.py through the gfx950 build, every case with LM_LOC_POISON unset and =1 (loc[] := 0 in front of the integrate
stage): byte-identical to each other, to the oracle and, where it models the document, to the plain merge model.  What the fiber
harness (tests/test_emu_loc_bitmap.py) cannot show is here: the bits are set by atomics that execute at L2 and read back by the same
wave — a window is looked up, an item in it is cut, an element behind the cut is looked up again (the windows corpus; the harness
test counts these lookups for the same documents)."""
import pytest

import _loc_bitmap_docs as D, _oracle, _resident

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def want():
    """the oracle's results per group, computed once (checked against the plain model where it is quick enough)"""
    out = {}
    for name, group in D.corpus().items():
        out[name] = _oracle.merge_batch([d for d, _ in group], threads=8)
        assert all(w[0] == 0 for w in out[name]), name
        n = 7 if name == "neighbours" else len(group)
        assert [D.model_result(reps) for _, reps in group[:n]] == out[name][:n], name
    return out


def _both(monkeypatch, run):
    monkeypatch.delenv("LM_LOC_POISON", raising=False)
    plain = run()
    monkeypatch.setenv("LM_LOC_POISON", "1")
    poisoned = run()
    assert plain == poisoned
    return plain


def _docs(*names):
    return [d for n in names for d, _ in D.corpus()[n]]


def test_window_edges(engine, want, monkeypatch):
    docs = _docs("edges", "edge_sessions")
    assert _both(monkeypatch, lambda: engine.merge_batch(docs)) == want["edges"] + want["edge_sessions"]


def test_lookup_cut_lookup_in_one_window(engine, want, monkeypatch):
    docs = _docs("windows", "fuzz") * 8   # (several waves per CU: other documents' bitmap lines pass through the same caches)
    assert _both(monkeypatch, lambda: engine.merge_batch(docs)) == (want["windows"] + want["fuzz"]) * 8


def test_neighbours_twice_in_one_context(engine, want, monkeypatch):
    docs = _docs("neighbours")
    order = [4, 8, 0, 6, 2, 7, 1, 5, 3]   # every slice moves

    def run():
        return engine.merge_batch(docs), engine.merge_batch([docs[i] for i in order]), engine.merge_batch(docs)
    first, second, third = _both(monkeypatch, run)
    assert first == want["neighbours"] and third == first and second == [first[i] for i in order]


@pytest.mark.parametrize("memset", ["1", "0"])
def test_retry_launch_replays_from_cleared_bits(engine, want, monkeypatch, memset):
    monkeypatch.setenv("LM_DIR_OPT_MAX", "4")
    monkeypatch.setenv("LM_LOC_MEMSET", memset)
    docs = _docs("retry", "edges")

    def run():
        got = engine.merge_batch(docs)
        assert engine.sizing()[3] >= 2, engine.sizing()   # documents the retry launch replayed: the two "retry" sessions at least
        return got
    assert _both(monkeypatch, run) == want["retry"] + want["edges"]


def test_resident_same_layout_and_renumbering(monkeypatch):
    import loro_amd
    sessions = [D.resident_session()]
    expect = _resident.oracle_sessions(sessions)
    assert all(w[0][0] == 0 for w in expect)
    fresh = []

    def run():
        with loro_amd.MergeEngine(0) as c:
            run0 = c.run

            def counting():
                run0()
                fresh.append(c.resident_fresh())
            c.run = counting
            return _resident.run_sessions(c, sessions)
    assert _both(monkeypatch, run) == expect
    n = len(sessions[0])
    assert fresh[0] == 1 and sum(fresh[1:n]) == 0, fresh   # every later run continues from the stored tracker (kept layout, then renumbered)


def test_mixed_batch(engine, monkeypatch):
    docs, fr = D.mixed_batch()
    expect = _oracle.merge_batch(docs, threads=8, frontiers=fr)
    assert all(w[0] == 0 for w in expect)
    for auto in ("1", "0"):   # the kernels the batch's statistics pick, and the span-granular kernels whatever they say
        monkeypatch.setenv("LM_SPAN_AUTO", auto)
        assert _both(monkeypatch, lambda: engine.merge_batch(docs, fr)) == expect
