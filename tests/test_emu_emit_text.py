"""The span-granular Text renderer (four elements per lane, escapes expanded in registers, an LDS window stored as aligned 16-byte
pieces) through the kernel-logic harness (tests/emu).  Expected bytes are the oracle's, and the plain merge model's (_merge_ref) for
every document: none is taken from an engine.  The documents and what they must contain: tests/_emit_text_docs.py."""
import pytest

import _emu, _emit_text_docs as D, _oracle, _resident
from loro_amd._cabi import Context


@pytest.fixture(scope="module")
def binding():
    return _emu.binding()


@pytest.fixture(scope="module")
def want():
    """the oracle's results per group, computed once and checked against the plain model"""
    out = {}
    for name, group in D.corpus().items():
        out[name] = _oracle.merge_batch([d for d, _ in group], threads=8)
        assert all(w[0] == 0 for w in out[name]), name
        assert [D.model_result(reps) for _, reps in group] == out[name], name
    return out


def _merge(binding, docs, fr=None):
    with Context(binding) as c:
        return c.merge_batch(docs, fr)


def _first_diff(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i, g[0], g[1][:120], w[1][:120]
    return None


def test_corpus_conditions():
    two, more, fallback, fast_esc = D.corpus_counts(D.corpus())
    print("lanes over two runs", two, "over three or four", more, "steps per element", fallback, "steps with a short escape", fast_esc)
    assert two >= 50 and more >= 20 and fallback >= 20 and fast_esc >= 20


@pytest.mark.parametrize("group", ["lengths", "runs", "escapes", "wide", "alignment"])
def test_group(binding, want, group, monkeypatch):
    monkeypatch.delenv("LM_SLAB_CAP", raising=False)
    docs = [d for d, _ in D.corpus()[group]]
    got = _merge(binding, docs)
    assert got == want[group], _first_diff(got, want[group])


def test_element_granular_agrees(binding, want, monkeypatch):
    monkeypatch.setenv("LM_SPAN", "0")
    for group in ("runs", "wide"):
        assert _merge(binding, [d for d, _ in D.corpus()[group]]) == want[group]


@pytest.mark.parametrize("cap", ["1", "64", "exact", "exact-1"])
def test_slab_overflow_one_document(binding, monkeypatch, cap):
    docs = [D.slab_edge_doc()]
    expect = _oracle.merge_batch(docs)
    n = len(expect[0][1])
    assert n % 16 == 1      # (a slab is a whole number of 16-byte pieces: one byte less is one piece less)
    monkeypatch.setenv("LM_SLAB_CAP", {"exact": str(n), "exact-1": str(n - 1)}.get(cap, cap))
    with Context(binding) as c:
        got = c.merge_batch(docs)
        reemits = c.sizing()[4]
    assert got == expect
    assert reemits == (0 if cap == "exact" else 1), (cap, n, reemits)


def test_slab_overflow_mixed_batch(binding, monkeypatch):
    docs = D.slab_docs()
    expect = _oracle.merge_batch(docs)
    lens = sorted(len(j) for _, j, *_ in expect)
    cap = lens[len(lens) // 2]
    monkeypatch.setenv("LM_SLAB_CAP", str(cap))
    with Context(binding) as c:
        got = c.merge_batch(docs)
        reemits = c.sizing()[4]
    assert got == expect
    assert reemits == sum(1 for n in lens if n > (cap + 15) // 16 * 16) and 0 < reemits < len(docs), (cap, lens, reemits)


def test_resident_checkout_uses_the_version_mask(binding):
    sessions = [D.version_session()]
    expect = _resident.oracle_sessions(sessions)
    assert all(w[0][0] == 0 for w in expect)
    assert len({w[0][1] for w in expect}) >= 2           # the versions render differently
    with Context(binding) as c:
        assert _resident.run_sessions(c, sessions) == expect
