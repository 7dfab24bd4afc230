"""Text / List deltas between two versions (lm_delta — LoroDoc::diff, the TextDelta / ListDiffItem events): k_delta_mark / k_delta's
logic through the host harness (tests/emu) against the plain reference derived from the oracle alone (_delta.py).  Every result is
compared byte for byte, then applied to the oracle's value at A; ctx.fetch() after the calls equals the result before them."""
import pytest

import _cursor, _delta, _emu, _fuzz, _oracle
from _delta import OK, TEXT, At
from loro_amd import wire
from loro_amd._cabi import Context


def ctx():
    return Context(_emu.binding())


@pytest.fixture(scope="module")
def corpus():
    docs, pairs = _delta.fuzz_corpus(range(24), n_steps=80)
    _delta.fuzz_condition(pairs)
    return docs, pairs


@pytest.mark.parametrize("span", ["1", "0", None])
def test_fuzz_documents_from_every_snapshot_version(monkeypatch, corpus, span):
    if span is not None:
        monkeypatch.setenv("LM_SPAN", span)
    docs, pairs = corpus
    with ctx() as c:
        assert _delta.run_fuzz(c, docs, pairs, "span=%s" % span) > 24 * 4


def test_hand_cases_and_statuses():
    with ctx() as c:
        _delta.run_hand_cases(c)
    with ctx() as c:
        c.stage([_delta.hand_cases()[0][1]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta([(0, None)])


def test_a_document_that_is_one_linear_chain(monkeypatch):
    monkeypatch.setenv("LM_CUT_MIN_ROWS", "0")
    with ctx() as c:
        _delta.run_chain(c, 400)


def test_more_than_one_pass_three_versions_and_sparse_queries():
    with ctx() as c:
        _delta.run_long_text(c)


def test_slab_overflow_takes_the_second_launch():
    with ctx() as c:
        _delta.run_overflow(c)


def test_only_the_written_bytes_cross_to_the_host():
    with ctx() as c:
        _delta.run_bytes_moved(c)


def test_the_self_check_refuses_when_status_and_id_sets_disagree(monkeypatch):
    with ctx() as c:
        _delta.run_self_check(c, monkeypatch)


@pytest.mark.parametrize("share", ["1", "0"])
def test_an_entry_rendered_at_a_checkout(monkeypatch, share):
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    (e1, _), (e2, f2), (e3, _) = _delta.steps()
    a, v, latest = At([e1]), At([e2]), At([e3])
    docs, fronts = [[e3], [e3]], [wire.encode_frontiers(f2), None]
    with ctx() as c:
        res = c.merge_batch(docs, fronts)
        assert res == _oracle.merge_batch(docs, frontiers=fronts)
        got = c.delta([(0, a.vv), (1, a.vv), (0, v.vv), (0, latest.vv)])
        _delta.check_one(got[0], a, v, 0, "checkout")
        _delta.check_one(got[1], a, latest, 0, "latest next to it")
        assert got[2][0] == OK and got[2][2] == b"{}"
        assert got[3][0] == _delta.FRONTIERS_NOT_FOUND          # A beyond the rendered version
        assert c.fetch() == res


def test_resident_flow():
    with ctx() as c:
        _delta.resident_flow(c, range(48), n=40)


def test_a_snapshot_staged_document():
    snaps = []
    reps = _fuzz.random_session(90, n_peers=3, n_steps=80, kinds=("text", "list"), snapshots=snaps)
    blobs = _fuzz.blobs_of(reps)
    full = wire.Replica(reps[0].peer)
    for r in reps:
        full.merge_from(r)
    st, ents = _oracle.state_entries([full.export()])
    assert st == 0
    snap = [full.export_snapshot(state=ents)]
    v = At(blobs)
    with ctx() as c:
        res = c.merge_batch([snap])
        assert c.b.state_documents(c.h) == 1 and res[0][:2] == _oracle.merge(blobs)[:2]
        vs = [At([]), At([snaps[0][1]]), At([snaps[-1][1]])]
        got = c.delta([(0, a.vv) for a in vs])
        for a, g in zip(vs, got):
            _delta.check_one(g, a, v, 0, "state-staged snapshot")
        assert c.fetch() == res
