"""GPU: the span-granular Text renderer of the gfx950 build — four elements per lane, escapes expanded in registers, an LDS window
stored as aligned 16-byte pieces — on the documents of tests/_emit_text_docs.py.  Expected bytes are the oracle's, checked against the
plain merge model; none is taken from an engine.  What the fiber harness (tests/test_emu_emit_text.py) does not model is here: the
prefix scan on the DPP crossbar in which every lane takes part, LDS addressed as window + offset by all lanes of a wave at once,
unaligned 32-bit loads and LDS stores, 16-byte stores to the slab, several waves of a CU each with a window of its own."""
import pytest

import _emit_text_docs as D, _oracle, _resident

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def want():
    """the oracle's results per group, computed once and checked against the plain model"""
    out = {}
    for name, group in D.corpus().items():
        out[name] = _oracle.merge_batch([d for d, _ in group], threads=8)
        assert all(w[0] == 0 for w in out[name]), name
        assert [D.model_result(reps) for _, reps in group] == out[name], name
    return out


def _first_diff(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i, g[0], g[1][:120], w[1][:120]
    return None


@pytest.mark.parametrize("group", ["lengths", "runs", "escapes", "wide", "alignment"])
def test_group(engine, want, group, monkeypatch):
    monkeypatch.delenv("LM_SLAB_CAP", raising=False)
    got = engine.merge_batch([d for d, _ in D.corpus()[group]])
    assert got == want[group], _first_diff(got, want[group])


@pytest.mark.parametrize("span", ["1", "0"])
def test_one_batch_of_everything(engine, want, monkeypatch, span):
    """several waves per CU, each with its own window; LM_SPAN=0: the element-granular leaves, which this renderer does not read"""
    monkeypatch.delenv("LM_SLAB_CAP", raising=False)
    monkeypatch.setenv("LM_SPAN", span)
    expect = [w for name in D.corpus() for w in want[name]] * 8
    got = engine.merge_batch(D.all_docs() * 8)
    assert got == expect, _first_diff(got, expect)


@pytest.mark.parametrize("cap", ["1", "64", "exact", "exact-1"])
def test_slab_overflow_one_document(engine, monkeypatch, cap):
    docs = [D.slab_edge_doc()]
    expect = _oracle.merge_batch(docs)
    n = len(expect[0][1])
    assert n % 16 == 1      # (a slab is a whole number of 16-byte pieces: one byte less is one piece less)
    monkeypatch.setenv("LM_SLAB_CAP", {"exact": str(n), "exact-1": str(n - 1)}.get(cap, cap))
    got = engine.merge_batch(docs)
    assert got == expect
    assert engine.sizing()[4] == (0 if cap == "exact" else 1), (cap, n, engine.sizing())


def test_slab_overflow_mixed_batch(engine, monkeypatch):
    docs = D.slab_docs()
    expect = _oracle.merge_batch(docs)
    lens = sorted(len(j) for _, j, *_ in expect)
    cap = lens[len(lens) // 2]
    monkeypatch.setenv("LM_SLAB_CAP", str(cap))
    got = engine.merge_batch(docs)
    reemits = engine.sizing()[4]
    assert got == expect
    assert reemits == sum(1 for n in lens if n > (cap + 15) // 16 * 16) and 0 < reemits < len(docs), (cap, lens, reemits)


def test_resident_checkout_uses_the_version_mask():
    import loro_amd
    sessions = [D.version_session()]
    expect = _resident.oracle_sessions(sessions)
    assert all(w[0][0] == 0 for w in expect)
    assert len({w[0][1] for w in expect}) >= 2           # the versions render differently
    with loro_amd.MergeEngine(0) as c:
        assert _resident.run_sessions(c, sessions) == expect
