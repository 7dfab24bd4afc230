"""GPU parity for lm_delta_richtext (Text deltas with style attributes from a version to the rendered one): k_rtdelta_mark / k_rtdelta
on the device through the C ABI against the plain reference derived from the merge model and the style rule alone
(_delta_richtext.py) — the cases of the kernel-logic harness (test_emu_delta_richtext.py), so the device runs exactly what the
harness ran."""
import pytest

import _delta_richtext
from loro_amd import wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    with loro_amd.MergeEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def corpus():
    docs = _delta_richtext.fuzz_docs()
    queries = _delta_richtext.fuzz_queries(docs)
    return docs, queries, _delta_richtext.check_conditions(docs, queries)


def test_hand_cases_and_statuses(engine):
    import loro_amd
    _delta_richtext.run_hand_cases(engine)
    with loro_amd.MergeEngine(0) as c:
        r = wire.Replica(5); r.text_insert("t", 0, "x"); r.commit()
        c.stage([[r.export()]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta_richtext([(0, None)])


def test_mark_boundaries_at_chunk_and_leaf_edges(engine):
    edges = _delta_richtext.edge_docs()
    assert _delta_richtext.run_edges(engine, edges) == 2 * len(edges)


def test_rt_max_marks_and_keys(engine):
    _delta_richtext.run_limits(engine, _delta_richtext.limit_docs())


def test_corpus(engine, corpus):
    docs, queries, _ = corpus
    assert _delta_richtext.run_docs(engine, docs, queries, "corpus", units=(0,)) == len(queries)


def test_slab_overflow_takes_the_second_launch(engine):
    _delta_richtext.run_overflow(engine)


def test_sixteen_versions_of_one_document_in_one_call(engine):
    assert _delta_richtext.run_many_versions(engine) == 16


def test_an_entry_rendered_at_a_checkout(engine):
    _delta_richtext.run_checkout(engine)


def test_resident_flow():
    import loro_amd
    with loro_amd.MergeEngine(0) as c:
        _delta_richtext.resident_flow(c)
