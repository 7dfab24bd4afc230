"""Map deltas between two versions (lm_delta_map — LoroDoc::diff, the MapDelta events): k_mdelta_mark / k_mdelta's logic through the
host harness (tests/emu) against the plain reference derived from the merge model alone (_delta_map.py).  Every result is compared
byte for byte, then applied to the shallow value of every Map at A; ctx.fetch() after the calls equals the result before them.

The corpora are _merge_docs_map.map_corpora(): "4 peers" from the empty version and every recorded version, "2 peers" from the empty
version and every fourth recorded version, "1-6 peers" from the empty version and every THIRD one (at every fourth it holds 49
"rewritten with an equal value" pairs, one short of the 50 asked for: more queries, not a lower threshold).  The GPU module takes all
three at every version.  The outcome thresholds are asserted, from the model alone, on exactly the queries this module sends."""
import pytest

import _delta_map, _emu, _merge_docs_map
from loro_amd import wire
from loro_amd._cabi import Context

# the settings of _merge_docs_map.SETTINGS that matter here: k_map_fused forced on (the documents are run once more through the row
# tables), k_map_fused off, the HBM builder's hash, retry tables
SETTINGS = [s for s in _merge_docs_map.SETTINGS if s[0] in ("fused", "LM_MAP_FUSED=0", "LM_LWW_LDS=0", "LM_HT_OPT=64")]
EVERY = {"2 peers": 4, "4 peers": 1, "1-6 peers": 3}


def ctx():
    return Context(_emu.binding())


@pytest.fixture(scope="module")
def corpora():
    out = {}
    for name, docs in _merge_docs_map.map_corpora().items():
        queries = _delta_map.corpus_queries(docs, EVERY[name])
        out[name] = (docs, queries, _delta_map.check_conditions(name, docs, queries))
    return out


def test_the_corpora_are_not_boring(corpora):
    assert len(SETTINGS) == 4
    for name, (docs, queries, counts) in corpora.items():
        print(name, len(queries), "queries", counts)
    assert len(corpora["4 peers"][1]) == 595                   # the empty version and every recorded version of every document


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
@pytest.mark.parametrize("name", ["2 peers", "4 peers", "1-6 peers"])
def test_corpus(monkeypatch, corpora, name, setting):
    label, env, fused_on, _ = setting
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    docs, queries, _ = corpora[name]
    with ctx() as c:
        assert _delta_map.run_corpus(c, docs, queries, "%s, %s" % (name, label), fused=fused_on and label == "fused") == len(queries)


def test_hand_cases_and_statuses():
    with ctx() as c:
        _delta_map.run_hand_cases(c)
    with ctx() as c:
        r = wire.Replica(5); r.map_set("m", "k", 1); r.commit()
        c.stage([[r.export()]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta_map([(0, None)])


def test_lane_groups_and_chunk_edges():
    with ctx() as c:
        _delta_map.run_shapes(c)


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_pairs_around_the_builder_switch(monkeypatch, setting):
    label, env, _, ht_opt = setting
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with ctx() as c:
        assert _delta_map.run_tables(c, ht_opt, label) == 3


def test_slab_overflow_takes_the_second_launch():
    with ctx() as c:
        _delta_map.run_overflow(c)


def test_only_the_written_bytes_cross_to_the_host():
    with ctx() as c:
        _delta_map.run_bytes_moved(c)


def test_the_self_check_refuses_when_the_winners_disagree(monkeypatch):
    with ctx() as c:
        _delta_map.run_self_check(c, monkeypatch)


@pytest.mark.parametrize("share", ["1", "0"])
def test_an_entry_rendered_at_a_checkout(monkeypatch, share):
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    with ctx() as c:
        _delta_map.run_checkout(c)


def test_resident_flow():
    with ctx() as c:
        _delta_map.resident_flow(c)


def test_a_snapshot_staged_document():
    with ctx() as c:
        _delta_map.run_snapshot(c)
