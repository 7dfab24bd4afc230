"""GPU parity for lm_delta_map (Map deltas from a version to the rendered one): k_mdelta_mark / k_mdelta on the device through the C
ABI against the plain reference derived from the merge model alone (_delta_map.py).  The cases of the kernel-logic harness
(test_emu_delta_map.py) with the three corpora at EVERY recorded version, plus the documents whose rows race for one table slot —
16 peers x 1,024 rows on 1, 2, 4 and 1,000 keys: the atomic_max64 contention the fiber harness cannot model."""
import pytest

import _delta_map, _merge_docs_map
from loro_amd import wire

pytestmark = pytest.mark.gpu

SETTINGS = [s for s in _merge_docs_map.SETTINGS if s[0] in ("fused", "LM_MAP_FUSED=0", "LM_LWW_LDS=0", "LM_HT_OPT=64")]


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
    for name, docs in _merge_docs_map.map_corpora().items():
        queries = _delta_map.corpus_queries(docs)
        out[name] = (docs, queries, _delta_map.check_conditions(name, docs, queries))
    return out


def test_the_corpora_are_not_boring(corpora):
    assert [len(corpora[n][1]) for n in ("2 peers", "4 peers", "1-6 peers")] == [1358, 595, 1016]


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
@pytest.mark.parametrize("name", ["2 peers", "4 peers", "1-6 peers"])
def test_corpus(engine, monkeypatch, corpora, name, setting):
    label, env, fused_on, _ = setting
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    docs, queries, _ = corpora[name]
    assert _delta_map.run_corpus(engine, docs, queries, "%s, %s" % (name, label), fused=fused_on and label == "fused") == len(queries)


@pytest.fixture(scope="module")
def races():
    return _merge_docs_map.race_docs()[0][2]


@pytest.mark.parametrize("from_first_peer", [False, True], ids=["A = empty", "A = the first peer's end"])
def test_rows_that_race_for_one_slot(engine, races, from_first_peer):
    res = engine.merge_batch([d.blobs for d in races])
    assert res == [d.model.result() for d in races]
    A = [{d.reps[0].peer: d.reps[0].vv[d.reps[0].peer]} if from_first_peer else {} for d in races]
    got = engine.delta_map([(i, wire.encode_vv(a)) for i, a in enumerate(A)])
    for d, a, g in zip(races, A, got):
        _delta_map.check_one(g, d.model, _delta_map.vv_ids(a), d.model.all_ids, d.label)
        # (65 blocks end with a block of the first peer alone: its end holds every winner)
        assert (g[2] != b"{}") == (not from_first_peer or d.label.startswith("32 blocks"))
    assert engine.fetch() == res


def test_hand_cases_and_statuses(engine):
    _delta_map.run_hand_cases(engine)
    with fresh() as c:
        r = wire.Replica(5); r.map_set("m", "k", 1); r.commit()
        c.stage([[r.export()]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta_map([(0, None)])


def test_lane_groups_and_chunk_edges(engine):
    _delta_map.run_shapes(engine)


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_pairs_around_the_builder_switch(engine, monkeypatch, setting):
    label, env, _, ht_opt = setting
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _delta_map.run_tables(engine, ht_opt, label) == 3


def test_slab_overflow_takes_the_second_launch(engine):
    _delta_map.run_overflow(engine)


def test_only_the_written_bytes_cross_to_the_host(engine):
    _delta_map.run_bytes_moved(engine)


def test_the_self_check_refuses_on_the_device(engine, monkeypatch):
    _delta_map.run_self_check(engine, monkeypatch)


def test_an_entry_rendered_at_a_checkout(engine):
    _delta_map.run_checkout(engine)


def test_resident_flow():
    with fresh() as c:
        _delta_map.resident_flow(c)


def test_a_snapshot_staged_document(engine):
    _delta_map.run_snapshot(engine)
