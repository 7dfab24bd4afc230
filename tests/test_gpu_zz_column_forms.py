"""GPU: the gfx950 build against the plain model on every legal column encoding (tests/_column_forms.py) — the documents and settings
of tests/test_column_forms.py through the product library.  What only the device has: LDS staging, col_var3's three unguarded LDS
loads at the end of a column, the slot arithmetic of blocks staged in part, the second launch with larger slots.  Every batch mixes
the forms: a document's canonical twin and its variants are neighbours, and the documents of 7, 8 and 9 blocks put blocks of
different forms into one wave's group of eight.  One engine and one set of documents per module."""
import pytest

import _column_forms as F, _merge_docs_map as M, _oracle

pytestmark = pytest.mark.gpu


def oracle(blobs):
    return _oracle.merge(blobs)


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def entries():
    corpus = F.corpus_entries()
    F.check_conditions(F.counts_of(corpus))
    return {"corpus": corpus, "hand": F.boundary_entries() + F.tail_entries() + F.width_entries() + F.dod_entries() + F.many_change_entries()}


def under(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS, ids=[s[0] for s in F.DECODER_SETTINGS])
def test_corpus(engine, entries, monkeypatch, setting):
    under(monkeypatch, setting[1])
    assert F.run_entries(engine, entries["corpus"], setting[0], oracle) == len(entries["corpus"])


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS, ids=[s[0] for s in F.DECODER_SETTINGS])
def test_hand_built_documents(engine, entries, monkeypatch, setting):
    under(monkeypatch, setting[1])
    assert F.run_entries(engine, entries["hand"], setting[0], oracle) == len(entries["hand"])


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_map_documents_keep_their_path(engine, monkeypatch, setting):
    """a form must not move a Map document off the fused path: fused_documents / redo_documents are the literals of _column_forms.MAP_PATHS"""
    name, env, fused_on, ht_opt = setting
    for big in ({}, {"LM_DEC_SLOT_BIG": "0"}):
        under(monkeypatch, dict(env, **big))
        assert F.check_map_paths(engine, name, oracle) == 68


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS[:4], ids=[s[0] for s in F.DECODER_SETTINGS[:4]])
def test_documents_in_steps(engine, monkeypatch, setting):
    """resident documents (stage + import_more, three steps): results after every step and resident_fresh() equal to the canonical run's"""
    under(monkeypatch, setting[1])
    assert F.check_steps(engine, setting[0]) >= 90


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS, ids=[s[0] for s in F.DECODER_SETTINGS])
def test_documents_inside_a_snapshot(engine, monkeypatch, setting):
    """the same blocks in the ChangeStore of a FastSnapshot whose state section holds placeholders: the history path"""
    under(monkeypatch, setting[1])
    ents = F.path_entries(", a snapshot", F.as_snapshot)
    assert F.run_snapshots(engine, ents, setting[0]) == len(ents) >= 90


def test_documents_beyond_the_limits(engine):
    F.check_limits(engine)
    F.check_message_sum(engine)


def test_zero_length_bool_runs(engine):
    """tests/test_column_forms.py::test_zero_length_bool_runs on the device: one F0 / T0 pair changes nothing, two and more are refused
    with LM_DECODE_ERROR — the oracle's verdict — and leave the neighbour in the batch alone"""
    for d in F.bool_docs():
        F.run_entries(engine, [(d, None)] + [(d, {"bool_rle": f}) for f in F.BOOL_ACCEPTED], "zero runs", oracle)
        got = engine.merge_batch([d.blobs({"bool_rle": f}) for f in F.BOOL_REFUSED] + [d.blobs()])
        assert all(g[:2] == (1, b"") for g in got[:-1]) and got[-1] == d.model.result(), [g[:2] for g in got]
