"""GPU parity for lm_delta_movable (MovableList deltas from a version to the rendered one): k_mldelta_mark / k_mldelta on the device
through the C ABI against the plain reference derived from the merge model alone (_delta_movable.py).  The cases of the kernel-logic
harness (test_emu_delta_movable.py), plus what the fiber harness cannot model: rows racing for one winner word — 8 peers, each moving
and setting the same 1, 2 and 64 elements 256 times (about 4,000 rows a document)."""
import pytest

import _delta_movable, _merge_docs
from loro_amd import wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


def fresh():
    import loro_amd
    return loro_amd.MergeEngine(0)


@pytest.fixture(scope="module")
def corpora():
    out = {}
    for name, docs in _merge_docs.movable_corpora().items():
        queries = _delta_movable.corpus_queries(docs)
        out[name] = (docs, queries, _delta_movable.check_conditions(name, docs, queries))
    return out


def test_the_corpora_are_not_boring(corpora):
    assert [len(corpora[n][1]) for n in ("movable", "movable nested", "movable 5 peers")] == [520, 299, 532]


@pytest.mark.parametrize("name", ["movable", "movable nested", "movable 5 peers"])
def test_corpus(engine, corpora, name):
    docs, queries, _ = corpora[name]
    assert _delta_movable.run_docs(engine, docs, queries, name) == len(queries)


@pytest.fixture(scope="module")
def races():
    return [_delta_movable.race_doc(n) for n in (1, 2, 64)]


@pytest.mark.parametrize("from_first_peer", [False, True], ids=["A = empty", "A = the first peer's end"])
def test_rows_that_race_for_one_winner_word(engine, races, from_first_peer):
    def a_of(d):
        if not from_first_peer:
            return []
        first = d.reps[1]
        return [(first.peer, first.vv[first.peer] - 1)]
    assert all(sum(len(c.ops) for c in d.model.changes) > 4000 for d in races)
    assert _delta_movable.run_docs(engine, races, [(i, a_of(d)) for i, d in enumerate(races)], "races") == 3


def test_hand_cases_and_statuses(engine):
    _delta_movable.run_hand_cases(engine)
    with fresh() as c:
        r = wire.Replica(5); r.mlist_insert("ml", 0, [1]); r.commit()
        c.stage([[r.export()]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta_movable([(0, None)])


def test_hand_built_documents_at_every_counter(engine):
    assert _delta_movable.run_hand_built(engine, _delta_movable.hand_built()) > 500


def test_runs_and_gaps_across_chunk_and_leaf_edges(engine):
    _delta_movable.run_row_passes(engine, _merge_docs.row_pass_docs())


def test_table_load_and_many_leaves(engine):
    _delta_movable.run_table_load(engine, _merge_docs.table_load_doc(1500))


def test_slab_overflow_takes_the_second_launch(engine):
    _delta_movable.run_overflow(engine)


def test_documents_without_a_movable_list(engine, monkeypatch):
    assert _delta_movable.run_without_a_movable_list(engine, monkeypatch) == 1        # the LWW Map document was decoded without op rows


def test_tree_and_counter_ops_set_bit_0(engine):
    _delta_movable.run_tree_and_counter_ops(engine)


def test_only_the_written_bytes_cross_to_the_host(engine):
    _delta_movable.run_bytes_moved(engine)


def test_the_self_check_refuses_on_the_device(engine, monkeypatch):
    _delta_movable.run_self_check(engine, monkeypatch)


def test_an_entry_rendered_at_a_checkout(engine):
    _delta_movable.run_checkout(engine)


def test_resident_flow():
    with fresh() as c:
        _delta_movable.resident_flow(c)


def test_a_snapshot_staged_document(engine):
    _delta_movable.run_snapshot(engine)
