"""GPU parity for lm_delta (Text / List deltas from a version to the rendered one): k_delta_mark / k_delta on the device through the
C ABI against the plain reference derived from the oracle alone (_delta.py).  The cases of the kernel-logic harness
(test_emu_delta.py) at larger sizes — the fiber harness does not model inactive lanes in permutes or LDS apertures — plus a
configs[1]-shaped document."""
import pytest

import _delta, _fuzz, _oracle
from _delta import OK, At
from loro_amd import wire, workload

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
def corpus():
    docs, pairs = _delta.fuzz_corpus(range(200, 400), n_steps=110)
    _delta.fuzz_condition(pairs)
    return docs, pairs


@pytest.mark.parametrize("span", ["1", "0", None])
def test_fuzz_documents_from_every_snapshot_version(engine, monkeypatch, corpus, span):
    if span is not None:
        monkeypatch.setenv("LM_SPAN", span)
    docs, pairs = corpus
    assert _delta.run_fuzz(engine, docs, pairs, "span=%s" % span) > 200 * 4


def test_hand_cases_and_statuses(engine):
    _delta.run_hand_cases(engine)
    with fresh() as c:
        c.stage([_delta.hand_cases()[0][1]])
        with pytest.raises(RuntimeError):             # before lm_run
            c.delta([(0, None)])


def test_a_document_that_is_one_linear_chain(engine):
    _delta.run_chain(engine, 3000)                    # above the 2,048-row threshold of the linear prefix


def test_more_than_one_pass_three_versions_and_sparse_queries(engine):
    _delta.run_long_text(engine)


def test_slab_overflow_takes_the_second_launch(engine):
    _delta.run_overflow(engine)


def test_only_the_written_bytes_cross_to_the_host(engine):
    _delta.run_bytes_moved(engine)


def test_the_self_check_refuses_when_status_and_id_sets_disagree(engine, monkeypatch):
    _delta.run_self_check(engine, monkeypatch)


def test_an_entry_rendered_at_a_checkout(engine):
    (e1, _), (e2, f2), (e3, _) = _delta.steps()
    a, v, latest = At([e1]), At([e2]), At([e3])
    docs, fronts = [[e3], [e3]], [wire.encode_frontiers(f2), None]
    res = engine.merge_batch(docs, fronts)
    assert res == _oracle.merge_batch(docs, frontiers=fronts)
    got = engine.delta([(0, a.vv), (1, a.vv), (0, v.vv), (0, latest.vv)])
    _delta.check_one(got[0], a, v, 0, "checkout")
    _delta.check_one(got[1], a, latest, 0, "latest next to it")
    assert got[2][0] == OK and got[2][2] == b"{}"
    assert got[3][0] == _delta.FRONTIERS_NOT_FOUND
    assert engine.fetch() == res


def test_resident_flow():
    with fresh() as c:
        _delta.resident_flow(c, range(48))


def test_a_snapshot_staged_document(engine):
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
    res = engine.merge_batch([snap])
    assert engine.b.state_documents(engine.h) == 1 and res[0][:2] == _oracle.merge(blobs)[:2]
    vs = [At([]), At([snaps[0][1]]), At([snaps[-1][1]])]
    for a, g in zip(vs, engine.delta([(0, a.vv) for a in vs])):
        _delta.check_one(g, a, v, 0, "state-staged snapshot")
    assert engine.fetch() == res


def test_a_configs1_shaped_document_from_the_end_of_its_base(engine):
    tpl = workload.Cfg2Template(5000, 2500, seed=0, commit_every=10, fuse=True)
    docs = [tpl.stamp(0), tpl.stamp(1)]
    res = engine.merge_batch(docs)
    assert res == _oracle.merge_batch(docs)
    for d, blobs in enumerate(docs):
        a, v = At(blobs[:1]), At(blobs)
        for units in (0, 1):
            _delta.check_one(engine.delta([(d, a.vv)], units)[0], a, v, units, ("cfg2", d))
    assert engine.fetch() == res
    # … and V = a checkout at the base's end: nothing changed
    a = At(docs[0][:1])
    vv = _delta._cursor.decode_vv(a.vv)
    fr = wire.encode_frontiers([(p, c - 1) for p, c in vv.items()])
    res = engine.merge_batch([docs[0]], [fr])
    assert res == _oracle.merge_batch([docs[0]], frontiers=[fr]) and res[0][2] == a.vv
    assert engine.delta([(0, a.vv)]) == [(OK, 0, b"{}")]
    assert engine.fetch() == res
