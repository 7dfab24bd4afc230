"""Text deltas with style attributes between two versions (lm_delta_richtext): k_rtdelta_mark / k_rtdelta's logic through the host
harness (tests/emu) against the plain reference derived from the merge model and the style rule alone (_delta_richtext.py).  Every
result is compared byte for byte, applied to the (scalar, attributes) pairs at A, and — its attributes stripped — compared with
lm_delta's answer to the same query; ctx.fetch() and ctx.richtext() after the calls equal their results before them.

The fuzz corpus is rich-text sessions queried from the empty version, every recorded version and versions that end between a
StyleStart and its StyleEnd; its floors are asserted, from the reference alone, before anything is compared.  Everything runs under
span leaves, LM_SPAN=0, LM_DECODE=0 and LM_DIR_OPT_MAX=4."""
import pytest

import _delta_richtext, _emu
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
def corpus():
    docs = _delta_richtext.fuzz_docs()
    queries = _delta_richtext.fuzz_queries(docs)
    return docs, queries, _delta_richtext.check_conditions(docs, queries)


@pytest.fixture(scope="module")
def edges():
    return _delta_richtext.edge_docs()


@pytest.fixture(scope="module")
def limits():
    return _delta_richtext.limit_docs()


def test_the_corpus_is_not_boring(corpus):
    docs, queries, counts = corpus
    print(len(queries), "queries", counts)
    assert all(counts[k] >= 20 for k in _delta_richtext.COUNTS[:-1]) and counts["undecided"] > 0


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_corpus(monkeypatch, corpus, env):
    setenv(monkeypatch, env)
    docs, queries, _ = corpus
    with ctx() as c:
        assert _delta_richtext.run_docs(c, docs, queries, env, units=(0, 1) if env == CONFIGS[0] else (0,)) == len(queries)


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_hand_cases_and_statuses(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_richtext.run_hand_cases(c)
    with ctx() as c:
        r = wire.Replica(5); r.text_insert("t", 0, "x"); r.commit()
        c.stage([[r.export()]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta_richtext([(0, None)])


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_mark_boundaries_at_chunk_and_leaf_edges(monkeypatch, edges, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        assert _delta_richtext.run_edges(c, edges) == 2 * len(edges)


@pytest.mark.parametrize("env", CONFIGS, ids=IDS)
def test_rt_max_marks_and_keys(monkeypatch, limits, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_richtext.run_limits(c, limits)


def test_slab_overflow_takes_the_second_launch():
    with ctx() as c:
        _delta_richtext.run_overflow(c)


def test_only_the_written_bytes_cross_to_the_host():
    with ctx() as c:
        _delta_richtext.run_bytes_moved(c)


@pytest.mark.parametrize("env", CONFIGS[:2], ids=IDS[:2])
def test_the_self_check_refuses(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_richtext.run_self_check(c, monkeypatch)


@pytest.mark.parametrize("env", [{"LM_SHARE_REPLAY": "1"}, {"LM_SHARE_REPLAY": "0"}, {"LM_SPAN": "0"}], ids=["share", "no share", "LM_SPAN=0"])
def test_an_entry_rendered_at_a_checkout(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_richtext.run_checkout(c)


@pytest.mark.parametrize("env", [CONFIGS[0], CONFIGS[3]], ids=[IDS[0], IDS[3]])      # (resident documents need the span-granular kernels)
def test_resident_flow(monkeypatch, env):
    setenv(monkeypatch, env)
    with ctx() as c:
        _delta_richtext.resident_flow(c)


def test_a_snapshot_staged_document():
    with ctx() as c:
        _delta_richtext.run_snapshot(c)


def test_sixteen_versions_of_one_document_in_one_call():
    with ctx() as c:
        assert _delta_richtext.run_many_versions(c) == 16
