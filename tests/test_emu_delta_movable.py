"""MovableList deltas between two versions (lm_delta_movable — LoroDoc::diff, the ListDiffItem events of a MovableList):
k_mldelta_mark / k_mldelta's logic through the host harness (tests/emu) against the plain reference derived from the merge model alone
(_delta_movable.py).  Every result is compared byte for byte, then applied to the shallow value of every MovableList at A;
ctx.fetch() after the calls equals the result before them.

The corpora are _merge_docs.movable_corpora() from the empty version and every recorded version (520 / 299 / 532 queries); the outcome
floors are asserted, from the model alone, before anything is compared.  Everything runs under the configurations of
test_merge_ref_movable.py: span leaves, LM_SPAN=0, LM_DECODE=0 and LM_DIR_OPT_MAX=4."""
import pytest

import _delta_movable, _emu, _merge_docs
from loro_amd import wire
from loro_amd._cabi import Context

CONFIGS = [{"LM_SPAN": "1"}, {"LM_SPAN": "0"}, {"LM_DECODE": "0"}, {"LM_DIR_OPT_MAX": "4"}]
IDS = [",".join("%s=%s" % kv for kv in e.items()) for e in CONFIGS]


def ctx():
    return Context(_emu.binding())


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def corpora():
    out = {}
    for name, docs in _merge_docs.movable_corpora().items():
        queries = _delta_movable.corpus_queries(docs)
        out[name] = (docs, queries, _delta_movable.check_conditions(name, docs, queries))
    return out


@pytest.fixture(scope="module")
def hand_built():
    return _delta_movable.hand_built()


@pytest.fixture(scope="module")
def row_passes():
    return _merge_docs.row_pass_docs()


@pytest.fixture(scope="module")
def table_load():
    return _merge_docs.table_load_doc(1500)


def test_the_corpora_are_not_boring(corpora):
    for name, (docs, queries, counts) in corpora.items():
        print(name, len(queries), "queries", counts)
    assert [len(corpora[n][1]) for n in ("movable", "movable nested", "movable 5 peers")] == [520, 299, 532]


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", ["movable", "movable nested", "movable 5 peers"])
def test_corpus(monkeypatch, corpora, name, env):
    setenv(monkeypatch, env)
    docs, queries, _ = corpora[name]
    with ctx() as c:
        assert _delta_movable.run_docs(c, docs, queries, (name, env)) == len(queries)


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_hand_cases_and_statuses(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_movable.run_hand_cases(c)
    with ctx() as c:
        r = wire.Replica(5); r.mlist_insert("ml", 0, [1]); r.commit()
        c.stage([[r.export()]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta_movable([(0, None)])


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_hand_built_documents_at_every_counter(monkeypatch, hand_built, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        assert _delta_movable.run_hand_built(c, hand_built, env) > 500


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_runs_and_gaps_across_chunk_and_leaf_edges(monkeypatch, row_passes, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_movable.run_row_passes(c, row_passes, env)


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_table_load_and_many_leaves(monkeypatch, table_load, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_movable.run_table_load(c, table_load, env)


def test_slab_overflow_takes_the_second_launch():
    with ctx() as c:
        _delta_movable.run_overflow(c)


def test_documents_without_a_movable_list(monkeypatch):
    with ctx() as c:
        assert _delta_movable.run_without_a_movable_list(c, monkeypatch) == 1        # the LWW Map document was decoded without op rows


def test_tree_and_counter_ops_set_bit_0():
    with ctx() as c:
        _delta_movable.run_tree_and_counter_ops(c)


def test_only_the_written_bytes_cross_to_the_host():
    with ctx() as c:
        _delta_movable.run_bytes_moved(c)


@pytest.mark.parametrize("env", CONFIGS[:2], ids=IDS[:2])
def test_the_self_check_refuses(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_movable.run_self_check(c, monkeypatch)


@pytest.mark.parametrize("env", [{"LM_SHARE_REPLAY": "1"}, {"LM_SHARE_REPLAY": "0"}, {"LM_SPAN": "0"}], ids=["share", "no share", "LM_SPAN=0"])
def test_an_entry_rendered_at_a_checkout(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_movable.run_checkout(c)


@pytest.mark.parametrize("env", [CONFIGS[0], CONFIGS[3]], ids=[IDS[0], IDS[3]])      # (resident documents need the span-granular kernels)
def test_resident_flow(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_movable.resident_flow(c)


def test_a_snapshot_staged_document():
    with ctx() as c:
        _delta_movable.run_snapshot(c)
