"""GPU parity for lm_delta against the definition restated over the plain merge model (tests/_delta_ref.py): k_delta_mark, k_delta and
k_delta_pack on the device on the corpora and the boundary documents of test_delta_ref.py — Text and List, root and child containers,
any pair of versions A inside V, checkouts, resident documents, documents that arrive in steps, a failed step, a document of zero op rows — under LM_SPAN=1, LM_SPAN=0 and
LM_SPAN_AUTO=1.  The kernel-logic harness does not model inactive lanes in permutes and ballots; the device does.  The floors are
asserted from the model (on the whole corpus) before anything runs; the versions asked are those of every third document (the CPU
module runs all of them), the hand-built documents run at full size.  No query may come back LM_UNSUPPORTED.

Time: 30 s for the module on an MI355X, 10 s of it the corpora and their models; the slowest test (linear prefix) 3 s."""
import pytest

import _cursor_ref as C, _delta, _delta_ref as R
from _delta import OK, FRONTIERS_NOT_FOUND
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
def corpus():
    docs = C.rich_docs(R.RICH_SEEDS) + C.nested_docs(R.NESTED_SEEDS)
    entries, chosen = R.entries_of(docs)
    counts = R.new_counts()
    R.expectations(entries, counts)
    counts.update({k: v for k, v in chosen.items() if k in counts})
    R.check_floors(counts)
    third, _ = R.entries_of(docs, every=3)
    return docs[::3], third, R.expectations(third)


@pytest.fixture(scope="module")
def boundary():
    entries = R.boundary_entries()
    return entries, R.expectations(entries)


@pytest.mark.parametrize("env", LAYOUTS + [("LM_SHARE_REPLAY", "0")], ids=lambda e: "%s=%s" % e)
def test_every_version_as_a_checkout_entry_from_every_chosen_version(engine, corpus, monkeypatch, env):
    monkeypatch.setenv(*env)
    _, entries, want = corpus
    assert R.run_entries(engine, entries, want, "%s=%s" % env) > 6000


@pytest.mark.parametrize("env", LAYOUTS, ids=lambda e: "%s=%s" % e)
def test_documents_on_the_kernels_boundaries(engine, boundary, monkeypatch, env):
    monkeypatch.setenv(*env)
    entries, want = boundary
    what = "boundaries, %s=%s" % env
    n = R.run_entries(engine, entries, want, what)
    n += R.run_asks(engine, entries, want, what + ", shuffled", order=1)
    assert n > 2000


def test_the_literals_on_the_device(engine):
    for name, d, a, v, exp, oc in R.literals():
        engine.merge_batch([d.blobs], None if v is None else [wire.encode_frontiers(v)])
        for units, e in exp.items():
            want = (FRONTIERS_NOT_FOUND, 0, b"") if e is None else (OK, oc, e)
            assert engine.delta([(0, wire.encode_vv(a))], units) == [want], (name, units)


def test_many_queries_on_one_document_duplicates_and_an_overflowing_slab(engine, boundary):
    d = C.leaf_docs()[1]
    assert engine.merge_batch([d.blobs]) == [d.model.result()]
    for n in (63, 64, 65, 129):
        frs = R.call_queries(d, n)
        got = engine.delta([(0, d.model.vv(fr)) for fr in frs], n & 1)
        for fr, g in zip(frs, got):
            R.check_one(g, R.Expect(d.model, d.model.version(fr), d.model.all_ids, n & 1), ("queries", n, fr))
    fr = R.call_queries(d, 40)[-1]
    got = engine.delta([(0, d.model.vv(fr))] * 70)
    assert len(set(got)) == 1
    R.check_one(got[0], R.Expect(d.model, d.model.version(fr), d.model.all_ids), "70 duplicates")
    # one slab overflows among many that do not: the second launch gives the same answers
    a_b, v_b = _delta.overflow_case()
    entries = [e for e in boundary[0] if e.frontiers is None][:40]
    engine.merge_batch([e.doc.blobs for e in entries] + [v_b])
    qs = [(k, a[2]) for k, e in enumerate(entries) for a in e.asks]
    alone = engine.delta(qs)
    both = engine.delta(qs + [(len(entries), _delta.At(a_b).vv)])
    assert both[:-1] == alone and both[-1][0] == OK and len(both[-1][2]) > 40000


def test_resident_documents_from_version_to_version(engine, corpus):
    assert R.run_resident(engine, corpus[0]) > 600


@pytest.mark.parametrize("env", [("LM_SPAN", "1"), ("LM_SPAN_AUTO", "1")], ids=lambda e: "%s=%s" % e)
def test_documents_that_arrive_in_steps(engine, monkeypatch, env):
    monkeypatch.setenv(*env)
    docs = C.step_docs()
    C.check_floors("steps", C.step_counts(docs), C.STEP_FLOORS)
    assert R.run_steps(engine, docs) > 500


def test_linear_prefix_sweep_and_backspace_documents(engine):
    entries = R.merge_docs_entries()
    latest = [e for e in entries if e.frontiers is None]
    assert R.run_entries(engine, latest, R.expectations(latest), "linear prefix, latest") > 100
    assert R.run_entries(engine, entries, R.expectations(entries), "linear prefix, every version") > 500


def test_a_fused_lww_map_document(engine):
    r = wire.Replica(90)
    for k in range(20):
        r.map_set("m", "k%d" % (k % 5), k); r.commit()
    d = C.Doc("maps only", [r])
    assert engine.merge_batch([d.blobs]) == [d.model.result()]
    got = engine.delta([(0, None), (0, wire.encode_vv({90: 7})), (0, wire.encode_vv({90: 20})), (0, wire.encode_vv({90: 21}))])
    assert got == [(OK, 1, b"{}"), (OK, 1, b"{}"), (OK, 0, b"{}"), (FRONTIERS_NOT_FOUND, 0, b"")]


def test_state_staged_snapshots_of_ten_rich_documents(engine):
    assert R.run_state_snapshots(engine, C.rich_docs(R.RICH_SEEDS[:10])) > 200


def test_the_status_after_a_failed_step_and_the_answers_from_the_version_that_survived(engine):
    R.run_failed_step(engine)


def test_a_document_of_zero_op_rows_between_two_queried_documents(engine):
    R.run_zero_row_document(engine)
