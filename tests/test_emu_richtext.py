"""Richtext values (lm_richtext; SURVEY §8f N4, second half — container/richtext/style_range_map.rs, richtext_state.rs:2500-2584,
state/richtext_state.rs:730-812): the oracle against the reference's known answers, and k_richtext's logic through the host harness
(tests/emu) against the oracle — batch documents under both integrate kernels, checkouts, resident documents step by step."""
import json

import pytest

import _emu, _fuzz, _oracle, _richtext, _richtext_ref
from loro_amd._cabi import Context


def test_oracle_gives_the_references_known_answers():
    for name, blobs, want in _richtext.known_answers():
        st, js = _oracle.richtext_batch([blobs])[0]
        assert st == 0, name
        assert json.loads(js) == {"cid:root-text:Text": want}, (name, js)


def test_oracle_gives_the_answer_the_reference_asserts_for_its_runtime_fixtures():
    """loro_js_interop.rs:86-94 — a reference-held richtext answer on reference-shipped blobs (updates and snapshot form)"""
    for name, blobs, want in _richtext.reference_held():
        st, js = _oracle.richtext_batch([blobs])[0]
        assert st == 4, name     # (Tree / Counter containers beside the Text: LM_UNSUPPORTED, everything in scope rendered)
        assert json.loads(js) == {"cid:root-text:Text": want}, (name, js)


def test_harness_gives_the_answer_the_reference_asserts_for_its_runtime_fixtures():
    ra = _richtext.reference_held()
    with Context(_emu.binding()) as c:
        c.merge_batch([b for _, b, _ in ra])
        got = c.richtext()
    for (name, _, want), (st, js) in zip(ra, got):
        assert json.loads(js) == {"cid:root-text:Text": want}, (name, st, js)
    # (the document's status is LM_UNSUPPORTED for its Tree / Counter containers; the richtext result has a status of its own)
    assert [j for _, j in got] == [j for _, j in _oracle.richtext_batch([b for _, b, _ in ra])]


def test_oracle_hand_cases_read_as_expected():
    got = {name: json.loads(_oracle.richtext_batch([blobs])[0][1]) for name, blobs in _richtext.hand_cases()}
    t = got["concurrent marks of one key"]["cid:root-text:Text"]
    # b's color mark (peer 20, same lamport region) wins where both apply; text is rendered once
    assert "".join(s["insert"] for s in t) == "0123456789"
    assert [s.get("attributes", {}).get("color") for s in t if "4" in s["insert"] or "5" in s["insert"]] == ["blue"]
    assert got["end anchor deleted"]["cid:root-text:Text"] == [{"insert": "abcdefgh"}]
    assert got["start anchor deleted"]["cid:root-text:Text"] == [{"insert": "abcdefgh"}]
    assert got["typing inside and at the edges"]["cid:root-text:Text"] == [{"insert": "aL"}, {"attributes": {"bold": True}, "insert": "bXc"}, {"insert": "Rd"}]
    # (entity positions: S1 S3 a E3 b S2 c d E2 e f E1 — "cd" carries two link ops with the same value: one span with "b" and "ef")
    assert got["equal values from different ops"]["cid:root-text:Text"] == [
        {"attributes": {"em": 1, "link": "u1"}, "insert": "a"}, {"attributes": {"link": "u1"}, "insert": "bcdef"}]
    # (a Text in which nothing is visible is not listed; one that holds only anchors is: its value is the empty list)
    assert got["several text containers"] == {"cid:root-only_anchors:Text": [], "cid:root-t2:Text": [{"insert": "plain \"text\"\n"}]}


def _harness(docs, fronts=None):
    with Context(_emu.binding()) as c:
        res = c.merge_batch(docs, fronts)
        return res, c.richtext()


@pytest.mark.parametrize("span", ["1", "0"])
def test_batch_documents_under_both_integrate_kernels(monkeypatch, span):
    monkeypatch.setenv("LM_SPAN", span)
    docs = [b for _, b, _ in _richtext.known_answers()] + [b for _, b in _richtext.hand_cases()] + _richtext.fuzz_docs(30) + _richtext.nested_docs(6)
    bad = [docs[0][0][:-2] + b"\x00\x01"]   # a document whose import fails: its richtext result carries that status
    docs.append(bad)
    res, got = _harness(docs)
    assert res == _oracle.merge_batch(docs)
    want = _oracle.richtext_batch(docs)
    assert want[-1][0] != 0
    _richtext.same(got, want, "span=" + span)
    assert sum(1 for s, b in got if b.count(b'"attributes"') >= 2) >= 15


def test_checkouts_cut_marks_at_every_op():
    docs, fronts = _richtext.checkout_cases()
    with Context(_emu.binding()) as c:
        import os
        os.environ["LM_SHARE_REPLAY"] = "0"     # (entries here have blob lists of their own anyway)
        try:
            res = c.merge_batch(docs, fronts)
            got = c.richtext()
        finally:
            del os.environ["LM_SHARE_REPLAY"]
    assert res == _oracle.merge_batch(docs, frontiers=fronts)
    _richtext.same(got, _oracle.richtext_batch(docs, frontiers=fronts), "checkout")


def test_resident_documents_step_by_step():
    sessions = _richtext.resident_sessions(range(6100, 6110))
    want = _richtext.oracle_resident(sessions)
    with Context(_emu.binding()) as c:
        got = _richtext.run_resident(c, sessions)
    for k, (g, w) in enumerate(zip(got, want)):
        ok = [(x[1], x[2]) if x[0] == 0 else (x[0], b"") for x in g]      # (a step whose checkout was refused: the fetch status says so)
        _richtext.same([o for o, x in zip(ok, g) if x[0] == 0], [y for y, x in zip(w, g) if x[0] == 0], "step %d" % k)


def test_a_folded_batch_is_unfolded_for_its_richtext_values():
    """entries that share their blobs (and, since round 6, every checked-out entry) are imported once and rendered by moving the
    trackers; lm_richtext needs the trackers AT every entry's version: the batch is unfolded — every entry a resident document over
    the bytes already uploaded — replayed, and gives the oracle's values (folding must not take API calls away)"""
    docs, fronts = _richtext.checkout_cases(n=2)
    shared = [docs[0]] * 3 + [docs[-1]] * 2
    fr = fronts[:3] + [fronts[-1], fronts[-3]]
    with Context(_emu.binding()) as c:
        res = c.merge_batch(shared, fr)
        assert c.b.shared_documents(c.h) == 2
        got = c.richtext()
        assert c.b.shared_documents(c.h) == 0
        assert c.fetch() == res      # (the same bytes after the unfolded run)
    assert res == _oracle.merge_batch(shared, frontiers=fr)
    _richtext.same(got, _oracle.richtext_batch(shared, fr), "folded")


def test_a_slab_that_is_too_small_sends_the_batch_through_a_second_launch(monkeypatch):
    docs = _richtext.fuzz_docs(8, base=5700)
    want = _oracle.richtext_batch(docs)
    monkeypatch.setenv("LM_RT_SLAB", "16")     # nothing fits: exact sizes come back, the second launch has room
    _, got = _harness(docs)
    _richtext.same(got, want, "slab 16")
    monkeypatch.delenv("LM_RT_SLAB")
    _, got = _harness(docs)
    _richtext.same(got, want, "default slab")


@pytest.mark.parametrize("auto", ["1"])   # (the suites' kernel choice "0": the GPU suite runs both)
def test_damaged_rich_text_documents_are_rendered_like_the_reference_or_rejected(monkeypatch, auto):
    """byte flips in documents full of marks and multi-byte scalars, under the suites' kernel choice and under the product default
    (LM_SPAN_AUTO=1: the element-granular kernel, whose deletes are now checked against the row's positions — 9 of these 400 documents
    used to come back with a value the reference does not compute) — and a damaged string in a PENDING change is an error as in the
    reference, which decodes every value of a block it reads."""
    monkeypatch.setenv("LM_SPAN_AUTO", auto)
    n_both, n_oracle_only = _richtext.check_damaged(_harness, _richtext.damaged_docs())
    assert n_both >= 40 and n_oracle_only <= (8 if auto == "0" else 24), (n_both, n_oracle_only)
    # (the seed-3 finding of the mixed corpus — a last lamport that does not fit u32 — is run on the GPU: test_gpu_zz_richtext.py)


@pytest.mark.parametrize("seed,auto", [(3, "1"), (5, "1"), (6, "0"), (901, "1")][1:])   # (901: a MovableList set row whose element's insert is not in its causal past, k_mlist_post)
def test_damaged_mixed_documents(monkeypatch, seed, auto):
    """the seeds on which the device used to give a verdict the reference does not give: two blocks whose last lamport does not fit
    (seed 3), a message-length column with a surplus run (seed 5), an insert row beyond the end (seed 6)"""
    monkeypatch.setenv("LM_SPAN_AUTO", auto)
    n_both, _ = _richtext.check_damaged(_harness, _richtext.damaged_mixed_docs(600, seed=seed))
    assert n_both >= 40


# ---- spans joined by VALUE: the oracle and the harness against the plain reference (tests/_richtext_ref.py)
def _session_orders(reps):
    """cid -> visible ids of every Text the replicas wrote, from the merged history (ordering has tests of its own)"""
    from loro_amd import wire
    blobs = _fuzz.blobs_of(reps)
    cids = {op.cid for c in _richtext_ref.changes_of(reps) for op in c.ops if op.cid.kind == wire.KIND_TEXT}
    return blobs, {cid: _oracle.visible_ids(blobs, cid, wire.KIND_TEXT) for cid in cids}


def test_value_pairs_are_what_the_reference_rule_says():
    pairs = _richtext.value_pairs()
    assert sum(1 for p in pairs if p[3]) == 11 and sum(1 for p in pairs if not p[3]) == 16


def test_oracle_against_the_plain_reference_on_the_value_corpus():
    cases = _richtext.value_corpus()
    assert len(cases) > 900
    _richtext.check_cases(_oracle.richtext_batch([c.blobs for c in cases]), cases, "oracle")
    # the corpus decides by value: in the touching placement an equal pair is ONE span showing the first value, an unequal pair two
    for name, v1, v2, eq in _richtext.value_pairs():
        for a, b in ((v1, v2), (v2, v1)):
            sp = _richtext_ref.spans(*(lambda c: (c.changes, _richtext.TEXT, c.order))(_richtext.placements(a, b)[0]))
            assert len(sp) == (1 if eq else 2) and sp[0][0]["c"] is a, name


def test_oracle_against_the_plain_reference_on_the_existing_corpora():
    """a third opinion on what the device is already compared with the oracle on: the rich fuzz sessions, the hand cases (deleted
    Start / End anchors, concurrent marks of one key, an unmark over part of a range, a Text that holds only anchors), the nested sessions"""
    sessions = [("fuzz %d" % i, r) for i, r in enumerate(_richtext.fuzz_sessions(30))] + _richtext.hand_sessions()
    sessions += [("nested %d" % i, r) for i, r in enumerate(_richtext.nested_sessions(6))]
    docs = _richtext.fuzz_docs(30) + [b for _, b in _richtext.hand_cases()] + _richtext.nested_docs(6)
    got = _oracle.richtext_batch(docs)
    for (name, reps), (st, js) in zip(sessions, got):
        _, orders = _session_orders(reps)
        assert st == 0 and js == _richtext_ref.richtext_bytes(_richtext_ref.changes_of(reps), orders), (name, js[:300])
    assert sum(js.count(b'"attributes"') for _, js in got) > 50


@pytest.mark.parametrize("span", ["1", "0"])
def test_harness_against_the_plain_reference(monkeypatch, span):
    monkeypatch.setenv("LM_SPAN", span)
    cases = _richtext.value_corpus()
    _, got = _harness([c.blobs for c in cases])
    _richtext.check_cases(got, cases, "span=" + span)


def test_harness_on_the_rows_the_corpus_was_asked_for():
    """abc marked c=v1, def c=v2: same bytes that are different maps (two spans, the second with ITS value), maps in another key order,
    two NaNs and the two zeros (one span), the infinities and NaN (two, although all print null), 1 and 1.0 (two)"""
    for row, cases in _richtext.table_rows():
        _, got = _harness([c.blobs for c in cases])
        _richtext.check_cases(got, cases, row)
        _richtext.check_cases(_oracle.richtext_batch([c.blobs for c in cases]), cases, "oracle " + row)


def test_harness_on_the_rows_when_no_slab_fits(monkeypatch):
    """three launches: k_richtext leaves the documents whose values need the walk, k_richtext_walk renders those, and because nothing
    fits into 16 bytes the whole batch — documents of both kinds — is rendered again at exact sizes"""
    monkeypatch.setenv("LM_RT_SLAB", "16")
    cases = [c for _, cs in _richtext.table_rows() for c in cs] + [c for n, c, _ in _richtext.limit_cases() if n.startswith("neighbour")][:1]
    _, got = _harness([c.blobs for c in cases])
    _richtext.check_cases(got, cases, "slab 16")


def test_harness_at_every_recorded_version_of_the_value_corpus():
    cases = _richtext.value_corpus()
    docs = _richtext.checkout_docs(cases)
    res, got = _harness([d[2] for d in docs], [d[3] for d in docs])
    assert all(r[0] == 0 for r in res)
    bad = [(cases[i].name, k, g) for (i, k, _, _), g in zip(docs, got) if g != (0, cases[i].want_at(k))]
    assert not bad, (len(bad), bad[:3])


def test_harness_when_the_second_mark_arrives_in_a_later_import():
    cases, sessions = _richtext.step_sessions(_richtext.value_corpus())
    assert len(cases) > 900
    with Context(_emu.binding()) as c:
        got = _richtext.run_resident(c, sessions)
    assert all(x[0] == 0 for step in got for x in step)
    bad = [(c.name, g) for c, g in zip(cases, got[0]) if (g[1], g[2]) != (0, c.want_at(0))]
    bad += [(c.name, g) for c, g in zip(cases, got[1]) if (g[1], g[2]) != (0, c.want)]
    assert not bad, (len(bad), bad[:3])


def test_harness_at_the_limits_of_the_style_tables():
    lim = _richtext.limit_cases()
    res, got = _harness([c.blobs for _, c, _ in lim])
    assert [r[0] for r in res] == [0] * len(lim)       # the documents themselves are fine: the limit is the rich-text result's alone
    assert [n for n, _, ok in lim if not ok] == ["65 open at one scalar", "65 distinct keys"]
    for (name, c, ok), g in zip(lim, got):
        assert g == (0, c.want) if ok else g[0] == 4, (name, g[0], g[1][:200])
