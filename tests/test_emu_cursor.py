"""Stable cursors (lm_cursor_pos / lm_cursor_at — LoroDoc::get_cursor_pos, loro.rs:1860-1994, state.rs:2061-2091; get_cursor,
handler.rs:2673-2735): k_cursor's logic through the host harness (tests/emu) against answers derived from the oracle alone
(_cursor.py).  Every generated query is compared, status included."""
import random

import pytest

import _cursor, _emu, _fuzz, _oracle
from _cursor import OK, DELETED, NOT_FOUND, DOC_FAILED, UNSUPPORTED, LEFT, MIDDLE, RIGHT, TEXT, LIST
from loro_amd import wire
from loro_amd._cabi import Context


def test_the_oracle_gives_tombstones_to_ask_for():
    """what _cursor.Expect relies on: the visible spans of lo_dump_spans are visible_ids, and every fuzz container holds tombstones"""
    for seed in range(6):
        blobs = _fuzz.blobs_of(_cursor.fuzz_session(seed))
        for name, kind in (("text", wire.KIND_TEXT), ("list", wire.KIND_LIST)):
            ex = _cursor.Expect(blobs, blobs, name, kind)
            assert len(ex.order) - len(ex.visible) >= 11, (seed, name)


@pytest.mark.parametrize("span", ["1", "0"])
def test_fuzz_documents_under_both_integrate_layouts(monkeypatch, span):
    monkeypatch.setenv("LM_SPAN", span)
    docs, pq, pw, aq, aw = _cursor.fuzz_corpus(range(24))
    assert sum(1 for w in pw if w[0] == DELETED) >= 24 * 2 * 11 and sum(1 for w in pw if w[0] == NOT_FOUND) >= 24 * 2 * 5
    with Context(_emu.binding()) as c:
        res = c.merge_batch(docs)
        assert res == _oracle.merge_batch(docs)
        n = _cursor.check(c, pq, pw, aq, aw, "span=" + span)
        assert c.fetch() == res          # the calls change nothing a run wrote
    assert n > 8000


def test_hand_cases_styled_astral_children_and_other_kinds():
    cases = _cursor.hand_cases()
    docs = [b for _, b, *_ in cases]
    bad = [docs[0][0][:-2] + b"\x00\x01"]            # a document whose import fails, next to healthy ones
    docs.append(bad)
    with Context(_emu.binding()) as c:
        res = c.merge_batch(docs)
        assert res == _oracle.merge_batch(docs) and res[-1][0] != 0

        def at(d, qs):
            return [(d,) + q[1:] for q in qs]
        pq, pw, aq, aw = [], [], [], []
        for d, (_, _, q, w, q2, w2) in enumerate(cases):
            pq += at(d, q); pw += w; aq += at(d, q2); aw += w2
        f = len(docs) - 1
        pq += [(f, TEXT, (7, 0), MIDDLE), (f, TEXT, None, RIGHT)]; pw += [(DOC_FAILED, 0, 0, MIDDLE), (DOC_FAILED, 0, 0, RIGHT)]
        aq += [(f, TEXT, 0, LEFT)]; aw += [(DOC_FAILED, None, LEFT, 0)]
        _cursor.check(c, pq, pw, aq, aw, "hand")
        assert c.fetch() == res
        with pytest.raises(RuntimeError):
            c.cursor_pos([(len(docs), TEXT, None, LEFT)])
    with Context(_emu.binding()) as c:
        c.stage(docs)
        with pytest.raises(RuntimeError):             # before lm_run
            c.cursor_pos([(0, TEXT, None, LEFT)])


@pytest.mark.parametrize("cut", [None, "0"])       # (the product's threshold for the prefix: 2,048 op rows; 0: every document)
def test_a_document_that_is_one_linear_chain(monkeypatch, cut):
    """the batch kernels replay such a history as a positional rope that drops what it deletes: the first cursor call runs the batch
    again without that prefix (same bytes out) and finds the tombstones"""
    if cut is not None:
        monkeypatch.setenv("LM_CUT_MIN_ROWS", cut)
    blobs = _cursor.chain_case(3000 if cut is None else 400)
    ex = _cursor.Expect(blobs, blobs, "text", wire.KIND_TEXT)
    assert len(ex.order) - len(ex.visible) > (300 if cut is None else 40)
    small = _fuzz.blobs_of(_cursor.fuzz_session(77))
    ex2 = _cursor.Expect(small, small, "list", wire.KIND_LIST)
    rng = random.Random(1)
    if cut is None:     # (a sample — tombstones among it — of the long chain, every id of the short one)
        pq, pw, aq, aw = _cursor.sample_queries(0, TEXT, ex, rng, 150)
    else:
        (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, ex, rng)
    assert sum(1 for w in pw if w[0] == DELETED) >= 37
    (q, w), (q2, w2) = _cursor.container_queries(1, LIST, ex2, rng)
    with Context(_emu.binding()) as c:
        res = c.merge_batch([blobs, small])
        assert res == _oracle.merge_batch([blobs, small])
        _cursor.check(c, pq + q, pw + w, aq + q2, aw + w2, "chain")
        assert c.fetch() == res
        c.run()                                       # the context stays without the prefix until the next lm_stage
        assert c.fetch() == res
        _cursor.check(c, pq[:200], pw[:200], aq[:50], aw[:50], "chain, second run")


def _stepwise(seed=5, n1=60, n2=60):
    """a single-writer history exported in steps: (blob at the intermediate version, its frontiers, full blob)"""
    rng = random.Random(seed)
    r = wire.Replica(31)

    def edit(n):
        for _ in range(n):
            ids = r.seq.setdefault(wire.root_cid("text", wire.KIND_TEXT), [])
            if ids and rng.random() < 0.35:
                pos = rng.randrange(len(ids))
                r.text_delete("text", pos, min(len(ids) - pos, rng.randint(1, 4)))
            else:
                r.text_insert("text", rng.randint(0, len(ids)), rng.choice(["ab", "c", "\U0001F600d", "xyz"]))
            if rng.random() < 0.3:
                r.commit()
        r.commit()
    edit(n1)
    mid, fr = r.export(), list(r.frontiers)
    edit(n2)
    return mid, fr, r.export()


@pytest.mark.parametrize("share", ["1", "0"])
def test_checkout_at_an_intermediate_version(monkeypatch, share):
    """ids created later are ID_NOT_FOUND, ids deleted later are OK at their old position; folded (the default: unfolded by the call)
    and as a batch entry that replays the version's causal closure (LM_SHARE_REPLAY=0)"""
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    mid, fr, full = _stepwise()
    at_v, latest = _cursor.Expect([full], [mid], "text", wire.KIND_TEXT), _cursor.Expect([full], [full], "text", wire.KIND_TEXT)
    later = [i for i in latest.order if i[1] >= at_v.vv[31]]
    deleted_later = [i for i in at_v.visible if i not in latest.vis]
    assert len(later) > 20 and len(deleted_later) > 10
    rng = random.Random(2)
    (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, at_v, rng)
    (q, w), (q2, w2) = _cursor.container_queries(1, TEXT, latest, rng)
    assert all(at_v.pos_answer(i, MIDDLE)[0] == NOT_FOUND for i in later) and all(at_v.pos_answer(i, MIDDLE)[0] == OK for i in deleted_later)
    docs, fronts = [[full], [full]], [wire.encode_frontiers(fr), None]
    with Context(_emu.binding()) as c:
        res = c.merge_batch(docs, fronts)
        assert res == _oracle.merge_batch(docs, frontiers=fronts)
        _cursor.check(c, pq + q, pw + w, aq + q2, aw + w2, "checkout share=" + share)
        assert c.fetch() == res


def test_resident_documents_a_caret_moves_by_the_concurrent_inserts_in_front_of_it():
    a, b = wire.Replica(41), wire.Replica(42)
    a.text_insert("text", 0, "hello world"); a.text_delete("text", 2, 2); a.commit()      # "heo world"
    first = a.export()
    b.merge_from(a); b.set_visible("text", wire.KIND_TEXT, _oracle.visible_ids([first], "text", wire.KIND_TEXT))
    b.text_insert("text", 0, "XYZ"); b.text_delete("text", 4, 1); b.commit()               # in front of the caret: +3, -1 ("XYZho world")
    a.text_insert("text", 9, "!"); a.commit()
    own_b = wire.Replica(42); own_b.changes = {42: b.changes[42]}
    second = [a.export(from_vv={41: a.changes[41][0].ctr_end}), own_b.export()]
    caret = (41, 6)                                                                        # 'w'
    e1, e2 = _cursor.Expect([first] + second, [first], "text", wire.KIND_TEXT), _cursor.Expect([first] + second, [first] + second, "text", wire.KIND_TEXT)
    rng = random.Random(3)
    with Context(_emu.binding()) as c:
        c.stage([[first]]); c.run()
        assert c.cursor_pos([(0, TEXT, caret, MIDDLE)]) == [(OK, 4, 4, MIDDLE)]
        (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, e1, rng)
        _cursor.check(c, pq, pw, aq, aw, "resident, first run")
        c.import_more([second]); c.run()
        res = c.fetch()
        assert res[0][:2] == _oracle.merge([first] + second)[:2]
        assert c.cursor_pos([(0, TEXT, caret, MIDDLE)]) == [(OK, 6, 6, MIDDLE)]
        (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, e2, rng)
        _cursor.check(c, pq, pw, aq, aw, "resident, after lm_import")
        assert c.fetch() == res
        # … and the resident document checked out at the first version again
        c.import_more([[]], [wire.encode_frontiers([(41, a.changes[41][0].ctr_end - 1)])]); c.run()
        (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, e1, rng)
        _cursor.check(c, pq, pw, aq, aw, "resident, checked out")


def test_state_staged_snapshots_and_folded_batches_answer_like_their_history_forms():
    reps = _cursor.fuzz_session(90)
    blobs = _fuzz.blobs_of(reps)
    full = wire.Replica(reps[0].peer)
    for r in reps:
        full.merge_from(r)
    st, ents = _oracle.state_entries([full.export()])
    assert st == 0
    snap = [full.export_snapshot(state=ents)]
    rng = random.Random(4)
    et, el = _cursor.Expect(blobs, blobs, "text", wire.KIND_TEXT), _cursor.Expect(blobs, blobs, "list", wire.KIND_LIST)
    (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, et, rng, el.order)
    (q, w), (q2, w2) = _cursor.container_queries(0, LIST, el, rng, et.order)
    pq += q; pw += w; aq += q2; aw += w2
    with Context(_emu.binding()) as c:
        res = c.merge_batch([snap])
        assert c.b.state_documents(c.h) == 1 and res[0][:2] == _oracle.merge(blobs)[:2]
        _cursor.check(c, pq, pw, aq, aw, "state-staged snapshot")
        assert c.fetch() == res
    # a folded batch: three entries over the same blobs, two of them checked out
    mid, fr, whole = _stepwise(seed=6)
    at_v, latest = _cursor.Expect([whole], [mid], "text", wire.KIND_TEXT), _cursor.Expect([whole], [whole], "text", wire.KIND_TEXT)
    doc = [whole]
    docs, fronts = [doc, doc, doc], [wire.encode_frontiers(fr), None, wire.encode_frontiers(fr)]
    pq, pw, aq, aw = [], [], [], []
    for d, ex in enumerate((at_v, latest, at_v)):
        (q, w), (q2, w2) = _cursor.container_queries(d, TEXT, ex, rng)
        pq += q; pw += w; aq += q2; aw += w2
    with Context(_emu.binding()) as c:
        res = c.merge_batch(docs, fronts)
        assert c.b.shared_documents(c.h) == 1
        _cursor.check(c, pq, pw, aq, aw, "folded")
        assert c.b.shared_documents(c.h) == 0 and c.fetch() == res


def test_more_queries_on_one_document_than_one_pass_holds():
    """64 queries ride in one pass over a container's leaves; 1,000 on one container take sixteen"""
    blobs = _fuzz.blobs_of(_cursor.fuzz_session(91, n_steps=300))
    ex = _cursor.Expect(blobs, blobs, "text", wire.KIND_TEXT)
    rng = random.Random(5)
    ids = [rng.choice(ex.order) for _ in range(1000)]
    pq = [(0, TEXT, i, rng.choice((LEFT, MIDDLE, RIGHT))) for i in ids]
    aq = [(0, TEXT, rng.randrange(ex.length + 2), MIDDLE) for _ in range(300)]
    with Context(_emu.binding()) as c:
        c.merge_batch([blobs])
        _cursor.check(c, pq, [ex.pos_answer(q[2], q[3]) for q in pq], aq, [ex.at_answer(q[2], q[3]) for q in aq], "chunks")
