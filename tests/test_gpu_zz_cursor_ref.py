"""GPU parity for lm_cursor_pos / lm_cursor_at against the cursor rules restated over the plain merge model (tests/_cursor_ref.py):
k_cursor on the device on the corpora and the boundary documents of test_cursor_ref.py — styled Text, child containers, every
recorded version three ways, documents that arrive in steps — under the default, LM_SPAN=0 and LM_SPAN_AUTO=1.  The kernel-logic
harness does not model inactive lanes in permutes; the device does.  Every floor is asserted from the model before anything runs.
The versions are those of every third document (the CPU module runs all of them).

Time: 15 s for the module on an MI355X, 4 s of it the corpora and their models; the slowest test (resident versions) 6 s."""
import pytest

import _cursor_ref as R
from _cursor import DELETED, LEFT, MIDDLE, RIGHT
from loro_amd import wire

pytestmark = pytest.mark.gpu

LAYOUTS = [("LM_SPAN", "1"), ("LM_SPAN", "0"), ("LM_SPAN_AUTO", "1")]


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpora():
    rich, nested, boundary = R.rich_docs(R.RICH_SEEDS), R.nested_docs(R.NESTED_SEEDS), R.boundary_docs()
    e = R.entries(rich)
    R.check_floors("rich", R.count(e[6], e[2], e[3]), R.RICH_FLOORS)
    e = R.entries(nested)
    assert sum(1 for q, w in zip(e[2], e[3]) if w[0] == DELETED and not q[1].startswith("cid:root-")) >= R.NESTED_FLOORS["deleted_in_children"]
    R.check_floors("versions", R.version_counts(rich + nested), R.VERSION_FLOORS)
    return rich, nested, boundary


@pytest.fixture(scope="module")
def latest(corpora):
    rich, nested, boundary = corpora
    return rich + nested + boundary, R.entries(rich + nested + boundary)


@pytest.fixture(scope="module")
def versions(corpora):
    docs = (corpora[0] + corpora[1])[::3]
    return docs, R.entries(docs, "all")


def run_batch(engine, e, what):
    blobs, fronts, pq, pw, aq, aw, _, want = e
    res = engine.merge_batch(blobs, fronts)
    assert res == want, what
    n = R.check(engine, pq, pw, aq, aw, what)
    assert engine.fetch() == res
    return n


@pytest.mark.parametrize("env", LAYOUTS, ids=lambda e: "%s=%s" % e)
def test_corpora_and_boundary_documents_at_the_latest_version(engine, latest, monkeypatch, env):
    monkeypatch.setenv(*env)
    docs, e = latest
    what = "%s=%s" % env
    blobs, fronts, pq, pw, aq, aw, _, want = e
    res = engine.merge_batch(blobs, fronts)
    assert res == want, what
    n = R.check(engine, pq, pw, aq, aw, what)
    for k, d in enumerate(docs):
        if d.label in ("one peer", "two peers", "255 peers"):
            q, w = R.peer_queries(k, d)
            n += R.check(engine, q, w, [], [], what + ", ids no element has")
        if d.label in ("three leaves", "a hole of leaves and a deleted tail"):
            for q, w in R.chunk_queries(k, d):
                n += R.check(engine, q, w, [], [], what + ", %d queries" % len(q))
    assert engine.fetch() == res
    assert n > 70000


def test_one_call_whose_queries_mix_documents_and_containers(engine, latest):
    """the host's sort branch and its scatter: every answer at its own index"""
    docs, e = latest
    blobs, fronts, pq, pw, aq, aw, _, want = e
    assert engine.merge_batch(blobs, fronts) == want
    R.check(engine, *R.shuffled(pq, pw, aq, aw), "shuffled")


@pytest.mark.parametrize("env", [("LM_SHARE_REPLAY", "1"), ("LM_SHARE_REPLAY", "0"), ("LM_SPAN", "0")], ids=lambda e: "%s=%s" % e)
def test_every_version_as_a_batch_entry(engine, versions, monkeypatch, env):
    monkeypatch.setenv(*env)
    assert run_batch(engine, versions[1], "versions, %s=%s" % env) > 50000


def test_every_version_of_resident_documents(engine, versions):
    assert R.run_resident_versions(engine, versions[0]) > 50000


@pytest.mark.parametrize("env", [("LM_SPAN", "1"), ("LM_SPAN_AUTO", "1")], ids=lambda e: "%s=%s" % e)
def test_documents_that_arrive_in_steps_at_both_versions_of_every_step(engine, monkeypatch, env):
    monkeypatch.setenv(*env)
    docs = R.step_docs()
    R.check_floors("steps", R.step_counts(docs), R.STEP_FLOORS)
    assert R.run_steps(engine, docs) > 10000


def test_literals_an_unreachable_child_a_child_without_an_op_and_the_root_limit(engine):
    d, pq, pw, aq, aw, ekey = R.unreachable_child_case()
    many = R.too_many_roots_doc()
    res = engine.merge_batch([d.blobs, many.blobs])
    assert res[0] == d.model.result() and res[1][0] == 4
    pq = pq + [(0, ekey, (5, 1), MIDDLE), (0, ekey, None, RIGHT), (1, "cid:root-t000:Text", (69, 0), MIDDLE), (1, "cid:root-t064:Text", None, RIGHT)]
    pw = pw + [(R.NO_CONTAINER, 0, 0, MIDDLE), (R.NO_CONTAINER, 0, 0, RIGHT), (R.UNSUPPORTED, 0, 0, MIDDLE), (R.UNSUPPORTED, 0, 0, RIGHT)]
    aq = aq + [(0, ekey, 0, MIDDLE), (1, "cid:root-t000:Text", 0, LEFT)]
    aw = aw + [(R.NO_CONTAINER, None, MIDDLE, 0), (R.UNSUPPORTED, None, LEFT, 0)]
    R.check(engine, pq, pw, aq, aw, "literals")


@pytest.mark.parametrize("share", ["1", "0"])
def test_a_container_in_front_of_its_first_op(engine, monkeypatch, share):
    """one leaf with nothing in it (`nr == 0` is unreachable: _cursor_ref.empty_container_case), as a batch entry and resident"""
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    d, fr, pq, pw, aq, aw = R.empty_container_case()
    res = engine.merge_batch([d.blobs, d.blobs], [wire.encode_frontiers(fr), None])
    assert res == [d.model.result(fr), d.model.result()]
    R.check(engine, pq, pw, aq, aw, "empty containers")
    engine.stage([d.blobs]); engine.run()
    engine.import_more([[]], [wire.encode_frontiers(fr)]); engine.run()
    R.check(engine, pq, pw, aq, aw, "empty containers, resident")


def test_state_staged_snapshots_of_ten_rich_documents(engine, corpora):
    import _oracle
    docs = corpora[0][:10]
    snaps = []
    for d in docs:
        full = wire.Replica(d.reps[0].peer)
        for r in d.reps:
            full.merge_from(r)
        st, ents = _oracle.state_entries([full.export()])
        assert st == 0
        snaps.append([full.export_snapshot(state=ents)])
    _, _, pq, pw, aq, aw, _, want = R.entries(docs)
    res = engine.merge_batch(snaps)
    assert engine.b.state_documents(engine.h) == 10 and [r[:2] for r in res] == [w[:2] for w in want]
    R.check(engine, pq, pw, aq, aw, "state-staged snapshots")
    assert engine.fetch() == res
