"""lm_delta (k_delta_mark, k_delta, k_delta_pack; Engine::delta_run / delta_slabs) through the kernel-logic harness against the
definition restated over the plain merge model (tests/_delta_ref.py): Text and List, root and child containers, styled Text, any
pair of versions A inside V — V a checkout, several heads, version vectors that are not causally closed —, documents that arrive in
steps, and documents built on the kernels' boundaries.  The expectation is the model's alone; every run's (status, JSON, version
vector, pending) must equal the model's before a delta is asked.  Every answer is compared byte for byte with its other_changed and
then applied (_delta.apply) to the model's value at A, per container.  No query on these legal documents may come back
LM_UNSUPPORTED.

Floors, asserted from the model before anything is compared (count seen over 30 rich + 30 nested sessions, 1,559 (document, V)
entries, 12,697 (A, V) pairs of which 12,078 have a V that is not the latest version; both units):
  containers with retain, insert and delete — child Text >= 200 (1,445), child List >= 200 (1,228), root List >= 200 (3,764);
  gaps with an insert behind a delete >= 500 (11,703); inserted child containers >= 500 (19,013); astral scalars in a retain or a
  delete >= 200 (9,323); multi-head A's >= 50 (485); multi-head V's >= 50 (60; the 24 + 24 seeds of _cursor_ref give 48, so six
  seeds were added to each corpus); {} with other_changed 1 >= 100 (251; the recorded versions alone give 4 in 4,733 pairs, so every V
  whose head ends in Map ops is also asked from the version in front of them) and with 0 >= 100 (1,163); elements hit by two delete
  atoms of V of which exactly one lies in A >= 100 (5,865); version vectors that are not causally closed >= 50 (1,305).
The large corpora run under the default setting only; LM_SPAN=0, LM_CUT_MIN_ROWS=0, LM_DIR_OPT_MAX=4 and LM_DECODE=0 run the boundary
documents and every version of _cursor_ref.small_version_docs.

LM_SHARE_REPLAY=1 runs every entry, =0 every other one.

Time: 462 s for the module in one process (the checkout entries 184 s shared and 48 s on their own, the four other settings 125 s).
"""
import pytest

import _cursor_ref as C, _delta, _delta_ref as R, _emu
from _delta import OK, FRONTIERS_NOT_FOUND
from loro_amd import wire
from loro_amd._cabi import Context


def ctx():
    return Context(_emu.binding())


# ------------------------------------------------------------------------------------------------------- the statement, before all
def test_the_statement_gives_every_hand_written_answer():
    """every literal of _delta.hand_cases() — "styled", "child text" and "list child" included, which _delta.expected skips — and the
    literals of _delta_ref.literals(), from the rules alone"""
    n = 0
    for name, model, A, exp, oc in R.hand_models():
        for units, e in exp.items():
            assert R.Expect(model, A, model.all_ids, units).answer() == (OK, oc, e), (name, units)
            n += 1
    assert n == 16
    m = 0
    for name, d, a, v, exp, oc in R.literals():
        for units, e in exp.items():
            want = (FRONTIERS_NOT_FOUND, 0, b"") if e is None else (OK, oc, e)
            assert R.Expect(d.model, R.vector_ids(a), d.model.version(v), units).answer() == want, (name, units)
            m += 1
    assert len(R.literals()) >= 30 and m >= 34


def test_the_escaper_is_the_json_of_a_text_value():
    import _values
    for s in _values.str_corpus():
        assert "".join(R.escape(c) for c in s) == _values.to_json(s)[1:-1], s


def test_the_statement_equals_the_oracle_derived_reference_on_its_own_corpus():
    """the corpus of test_emu_delta.py (oracle-written, unstyled, two roots): the statement over the model of the same writers gives
    _delta.expected's bytes — the restatement against the oracle, without the harness"""
    import _fuzz, _richtext_ref
    n = 0
    for seed in range(24):
        snaps = []
        reps = _fuzz.random_session(seed, n_peers=3, n_steps=80, kinds=("text", "list"), snapshots=snaps)
        m = R._merge_ref.Model(_richtext_ref.changes_of(reps))
        v = _delta.At(_fuzz.blobs_of(reps))
        for fr, upd in [([], None)] + snaps:
            a = _delta.At([upd] if upd else [])
            for units in (0, 1):
                assert R.Expect(m, m.version(fr) if fr else frozenset(), m.all_ids, units).bytes == _delta.expected(a, v, units)[0], (seed, fr, units)
                n += 1
    assert n > 24 * 4 * 2


# -------------------------------------------------------------------------------------------------------------------- the corpora
@pytest.fixture(scope="module")
def corpus():
    docs = C.rich_docs(R.RICH_SEEDS) + C.nested_docs(R.NESTED_SEEDS)
    entries, chosen = R.entries_of(docs)
    counts = R.new_counts()
    want = R.expectations(entries, counts)
    counts.update({k: v for k, v in chosen.items() if k in counts})
    R.check_floors(counts)
    return docs, entries, want


def _slices(entries, want, n):
    for lo in range(0, len(entries), n):
        yield entries[lo:lo + n], {u: w[lo:lo + n] for u, w in want.items()}


@pytest.mark.parametrize("share", ["1", "0"])
def test_every_version_as_a_checkout_entry_from_every_chosen_version(corpus, monkeypatch, share):
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    _, entries, want = corpus
    if share == "0":                                   # every entry shares its replay; every other one also runs on its own
        entries, want = entries[::2], {u: w[::2] for u, w in want.items()}
    n = 0
    for es, w in _slices(entries, want, 400):
        with ctx() as c:
            n += R.run_entries(c, es, w, "LM_SHARE_REPLAY=" + share)
    assert n > (20000 if share == "1" else 10000)


def test_resident_documents_from_version_to_version(corpus):
    with ctx() as c:
        assert R.run_resident(c, corpus[0]) > 2000


def test_documents_that_arrive_in_steps():
    docs = C.step_docs()
    C.check_floors("steps", C.step_counts(docs), C.STEP_FLOORS)
    with ctx() as c:
        assert R.run_steps(c, docs) > 500


def test_the_status_after_a_failed_step_and_the_answers_from_the_version_that_survived():
    with ctx() as c:
        R.run_failed_step(c)


def test_a_document_of_zero_op_rows_between_two_queried_documents():
    with ctx() as c:
        R.run_zero_row_document(c)


def test_state_staged_snapshots_of_ten_rich_documents(corpus):
    with ctx() as c:
        assert R.run_state_snapshots(c, corpus[0][:10]) > 200


def test_linear_prefix_sweep_and_backspace_documents():
    """a batch with a document that went through the linear prefix is run once more keeping its tombstones (loro_merge.h:449)"""
    entries = R.merge_docs_entries()
    latest = [e for e in entries if e.frontiers is None]
    with ctx() as c:
        assert R.run_entries(c, latest, R.expectations(latest), "linear prefix, latest") > 100
    with ctx() as c:
        assert R.run_entries(c, entries, R.expectations(entries), "linear prefix, every version") > 500


def test_a_fused_lww_map_document():
    """a document of Map containers only: {} with other_changed == (A != V)"""
    r = wire.Replica(90)
    for k in range(20):
        r.map_set("m", "k%d" % (k % 5), k); r.commit()
    d = C.Doc("maps only", [r])
    with ctx() as c:
        assert c.merge_batch([d.blobs]) == [d.model.result()]
        got = c.delta([(0, None), (0, wire.encode_vv({90: 7})), (0, wire.encode_vv({90: 20})), (0, wire.encode_vv({90: 21}))])
        assert got == [(OK, 1, b"{}"), (OK, 1, b"{}"), (OK, 0, b"{}"), (FRONTIERS_NOT_FOUND, 0, b"")]


# --------------------------------------------------------------------------------------------------------------------- boundaries
@pytest.fixture(scope="module")
def boundary():
    entries = R.boundary_entries()
    return entries, R.expectations(entries)


def run_boundary(boundary, what):
    entries, want = boundary
    with ctx() as c:
        n = R.run_entries(c, entries, want, what)
        n += R.run_asks(c, entries, want, what + ", shuffled", order=1)
    return n


def test_documents_on_the_kernels_boundaries(boundary):
    assert run_boundary(boundary, "boundaries") > 2000


def test_the_literals_on_the_harness():
    for name, d, a, v, exp, oc in R.literals():
        with ctx() as c:
            c.merge_batch([d.blobs], None if v is None else [wire.encode_frontiers(v)])
            for units, e in exp.items():
                want = (FRONTIERS_NOT_FOUND, 0, b"") if e is None else (OK, oc, e)
                assert c.delta([(0, wire.encode_vv(a))], units) == [want], (name, units)


def test_many_queries_on_one_document_and_duplicates():
    """63 / 64 / 65 / 129 queries with different A on one document, 70 duplicates"""
    d = C.leaf_docs()[1]
    with ctx() as c:
        assert c.merge_batch([d.blobs]) == [d.model.result()]
        for n in (63, 64, 65, 129):
            frs = R.call_queries(d, n)
            got = c.delta([(0, d.model.vv(fr)) for fr in frs], n & 1)
            for fr, g in zip(frs, got):
                R.check_one(g, R.Expect(d.model, d.model.version(fr), d.model.all_ids, n & 1), ("queries", n, fr))
        fr = R.call_queries(d, 40)[-1]
        got = c.delta([(0, d.model.vv(fr))] * 70)
        assert len(set(got)) == 1
        R.check_one(got[0], R.Expect(d.model, d.model.version(fr), d.model.all_ids), "70 duplicates")


def test_one_slab_overflows_among_many_that_do_not(boundary):
    """the second launch gives the same answers: every boundary query next to the overflowing one of _delta.overflow_case"""
    a_b, v_b = _delta.overflow_case()
    entries, want = boundary
    entries = [e for e in entries if e.frontiers is None][:40]
    with ctx() as c:
        c.set_profiling(1)
        docs = [e.doc.blobs for e in entries] + [v_b]
        c.merge_batch(docs)
        qs = [(k, a[2]) for k, e in enumerate(entries) for a in e.asks]
        alone = c.delta(qs)
        assert [n for n, _ in c.kernel_times()].count("k_delta") == 1
        both = c.delta(qs + [(len(entries), _delta.At(a_b).vv)])
        assert [n for n, _ in c.kernel_times()].count("k_delta") == 1 + 2        # (the times add up over the calls of one run)
        assert both[:-1] == alone and both[-1][0] == OK and len(both[-1][2]) > 40000
        c.set_profiling(0)


SETTINGS = [("LM_SPAN", "0"), ("LM_CUT_MIN_ROWS", "0"), ("LM_DIR_OPT_MAX", "4"), ("LM_DECODE", "0")]


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: "%s=%s" % e)
def test_small_corpus_and_boundaries_under_other_settings(boundary, monkeypatch, env):
    monkeypatch.setenv(*env)
    what = "%s=%s" % env
    run_boundary(boundary, "boundaries, " + what)
    small = C.small_version_docs()
    entries, _ = R.entries_of(small)
    want = R.expectations(entries)
    for share in ("1", "0"):
        monkeypatch.setenv("LM_SHARE_REPLAY", share)
        with ctx() as c:
            R.run_entries(c, entries, want, "small, %s, LM_SHARE_REPLAY=%s" % (what, share))
    monkeypatch.delenv("LM_SHARE_REPLAY")
    if env[0] != "LM_SPAN":
        with ctx() as c:
            R.run_resident(c, small, "resident, " + what)
