"""The plain merge model (tests/_merge_ref.py: sequence order by the sibling rule of crdt_rope.rs, deletes by position, Map LWW,
child containers, checkout — no oracle, kernel or tracker code) against
  (a) the reference's own known answers: the fugue.rs scripts and the test.rs checkouts that test_oracle_golden.py pins the oracle on;
  (b) the oracle: JSON bytes, version vector bytes and the visible ids of every sequence container, at the latest version and at
      every recorded version, on corpora whose writers took their views from the MODEL (no decision of the oracle in them);
  (c) the kernel-logic harness under every integrate instantiation, with and without the node cut;
  (d) lm_delta and lm_cursor_pos with expectations whose ids come from the model.
Before anything is compared, every corpus must show each outcome of the sibling rule often enough (_merge_docs.check_conditions).

LM_PLAIN chooses among the instantiations for DF_PLAIN documents only, and the host clears DF_PLAIN for a checked-out document
(lm_pipeline.h "rendered at the latest version"): checkouts run under LM_PLAIN unset and LM_SPAN=0, latest versions under all.

Time.  129 s for the module in one process on an 8-thread host (test_values.py: 54 s): the corpora and their models 7 s, (a) + (b) 8 s,
(d) 4 s, the hand-built documents 25 s, and the eight harness configurations 9 - 12 s each, 85 s together — (c) is 160 documents x 8
configurations + 160 checkouts x 4, at about 0.035 s per document in the harness.  (With glibc's swapcontext under the harness's fibers
the module took 578 s, a document 0.25 s: lm_wave.h switches fibers itself since.)  What was left to this module is small: the corpora
beyond the first at the fewest seeds, in steps of ten, that meet the outcome counts; one checkout per document in (c); each
configuration is a test of its own, so pytest-xdist spreads them."""
import pytest

import _cursor, _delta, _emu, _merge_docs, _merge_ref, _oracle
from _richtext_ref import changes_of
from loro_amd import wire
from loro_amd._cabi import Context

TEXT = _merge_docs.TEXT


def model_of(*reps):
    return _merge_ref.Model(changes_of(reps))


@pytest.fixture(scope="module")
def corpora():
    out = _merge_docs.corpora()
    for name, docs in out.items():
        _merge_docs.check_conditions(name, docs)
    return out


# ------------------------------------------------------------------------------------------- (a) the reference's own answers
def test_fugue_scripts():
    """crates/loro-internal/tests/fugue.rs:5-90, the scripts of test_oracle_golden.py:72-120"""
    a = wire.Replica(0); a.text_insert("text", 0, "Hello"); a.commit()
    b = wire.Replica(1); b.text_insert("text", 0, " World!"); b.commit()
    assert model_of(a, b).value() == {"text": "Hello World!"}
    a = wire.Replica(0)
    for ch in "olleH":
        a.text_insert("text", 0, ch)
    a.commit()
    b = wire.Replica(1)
    for ch in "!dlroW ":
        b.text_insert("text", 0, ch)
    b.commit()
    assert model_of(a, b).value() == {"text": "Hello World!"}
    a = wire.Replica(0); a.text_insert("text", 0, "ll"); a.text_insert("text", 0, "He"); a.text_insert("text", 4, "o"); a.commit()
    b = wire.Replica(1); b.text_insert("text", 0, " !"); b.text_insert("text", 1, "W")
    for ch in "dlro":
        b.text_insert("text", 2, ch)
    b.commit()
    assert model_of(a, b).value() == {"text": "Hello World!"}
    a, b, c = wire.Replica(0), wire.Replica(1), wire.Replica(2)
    c.text_insert("text", 0, "2"); c.commit()
    a.merge_from(c); a.set_visible("text", wire.KIND_TEXT, _merge_ref.view(a, TEXT))
    a.text_insert("text", 0, "1"); a.commit()
    b.text_insert("text", 0, "b"); b.commit()
    m = model_of(a, b, c)
    assert m.value() == {"text": "b12"} and m.json() == b'{"text":"b12"}'


def test_map_lww_peer_tiebreak_and_delete():
    """equal lamports: the larger peer wins (delta/map_delta.rs:26-32); a delete competes like a write (map_state.rs:438-449)"""
    a = wire.Replica(5); a.map_set("map", "k", "from5"); a.map_set("map", "gone", 1); a.commit()
    b = wire.Replica(9); b.map_set("map", "k", "from9"); b.map_delete("map", "gone"); b.commit()
    assert model_of(a, b).value() == {"map": {"k": "from9"}}


def test_text_checkout_known_answers():
    """test.rs:518-585 `test_text_checkout`"""
    r = wire.Replica(1)
    r.text_insert("text", 0, "你界")
    r.text_insert("text", 1, "好世")
    r.commit()
    m = model_of(r)
    for ctr, want in enumerate(["你", "你界", "你好界", "你好世界"]):
        assert m.value([(1, ctr)]) == {"text": want} and m.vv([(1, ctr)]) == wire.encode_vv({1: ctr + 1})
    r.text_delete("text", 3, 1)
    r.text_delete("text", 2, 1)
    r.commit()
    m = model_of(r)
    assert m.value() == {"text": "你好"}
    for ctr, want in [(3, "你好世界"), (4, "你好世"), (5, "你好"), (0, "你"), (1, "你界"), (2, "你好界")]:
        assert m.value([(1, ctr)]) == {"text": want}
    assert m.result([]) == (0, b'{"text":""}', wire.encode_vv({}), 0)


def test_map_checkout_known_answers():
    """test.rs:587-603 `map_checkout` and :659-693 `map_concurrent_checkout`"""
    r = wire.Replica(5)
    r.map_set("meta", "key", 0); r.commit()
    r.map_set("meta", "key", 1); r.commit()
    m = model_of(r)
    assert m.value([(5, 0)]) == {"meta": {"key": 0}} and m.value([]) == {"meta": {}} and m.value([(5, 1)]) == {"meta": {"key": 1}}
    a, b = wire.Replica(1), wire.Replica(2)
    a.map_set("meta", "key", 0); a.commit()
    va = list(a.frontiers)
    b.map_set("meta", "s", 1); b.commit()
    vb0 = list(b.frontiers)
    b.map_set("meta", "key", 1); b.commit()
    vb1 = list(b.frontiers)
    a.merge_from(b)
    a.map_set("meta", "key", 2); a.commit()
    vm = list(a.frontiers)
    m = model_of(a)
    for v, want in [(va, {"key": 0}), (vb0, {"s": 1}), (vb1, {"s": 1, "key": 1}), (vm, {"s": 1, "key": 2}), (va + vb1, {"s": 1, "key": 1})]:
        assert m.value(v) == {"meta": want}


def test_root_containers_the_state_store_holds():
    """the expectations of _cases.container_existence_cases (diff_calc.rs:299, state.rs:1352-1391), from the writers' changes"""
    a = wire.Replica(1)
    a.text_insert("text", 0, "ab"); a.list_insert("list", 0, [1, 2]); a.map_set("map", "k", 1); a.commit(); v1 = list(a.frontiers)
    a.text_delete("text", 0, 2); a.list_delete("list", 0, 2); a.map_delete("map", "k"); a.commit(); v2 = list(a.frontiers)
    m = model_of(a)
    assert m.json() == m.json(v2) == m.json([]) == b'{"map":{}}'
    assert m.json(v1) == b'{"list":[1,2],"map":{"k":1},"text":"ab"}'
    a.text_insert("text", 0, "c"); a.commit()
    m = model_of(a)
    assert m.json() == b'{"map":{},"text":"c"}' and m.json(v2) == m.json([]) == b'{"map":{},"text":""}'
    p, q, r = wire.Replica(11), wire.Replica(12), wire.Replica(13)
    p.text_insert("text", 0, "abc"); p.commit(); vp = list(p.frontiers)
    for x in (q, r):
        x.merge_from(p)
        x.set_visible("text", wire.KIND_TEXT, _merge_ref.view(x, TEXT))
        x.text_delete("text", 0, 2); x.commit()
    q.merge_from(r)
    m = model_of(q)
    assert m.json() == b'{"text":"c"}' and m.json([]) == b'{"text":""}'
    q.set_visible("text", wire.KIND_TEXT, _merge_ref.view(q, TEXT))
    q.text_delete("text", 0, 1); q.commit()
    m = model_of(q)
    assert m.json() == m.json([]) == b"{}" and m.json(vp) == b'{"text":"abc"}'


def test_a_reversed_delete_run_cut_by_a_checkout():
    """backspacing merges into one DeleteSpan of negative length (list_op.rs:396-423); atom i of it hits the i-th element from the
    RIGHT (DeleteSpanWithId::slice, list_op.rs:251-277): a version that holds two of its three atoms shows the leftmost target"""
    r = wire.Replica(3)
    r.text_insert("text", 0, "abcde"); r.commit()
    for pos in (3, 2, 1):
        r.text_delete("text", pos, 1)
    r.commit()
    op = r.changes[3][1].ops[0]
    assert op.signed_len == -3 and len(r.changes[3][1].ops) == 1
    m = model_of(r)
    blobs = [r.export()]
    for ctr, want in ((4, "abcde"), (5, "abce"), (6, "abe"), (7, "ae")):
        assert m.value([(3, ctr)]) == {"text": want}
        assert _oracle.merge(blobs, frontiers=wire.encode_frontiers([(3, ctr)])) == m.result([(3, ctr)])


# ------------------------------------------------------------------------------------------- (b) the model against the oracle
@pytest.mark.parametrize("name", ["3 peers", "5 peers", "with map", "styles", "nested"])
def test_model_against_oracle(corpora, name):
    docs = corpora[name]
    blobs = [d.blobs for d in docs]
    for d, got in zip(docs, _oracle.merge_batch(blobs, threads=8)):
        assert got == d.model.result(), (d.label, got, d.model.result())
        for cid in d.model.sequences():
            assert _oracle.visible_ids(d.blobs, cid, cid.kind) == d.model.visible_ids(cid), (d.label, cid)
    at = [(d, fr, upd) for d in docs for fr, upd in d.snaps] + [(d, fr, None) for d in docs for fr in d.versions]
    got = _oracle.merge_batch([d.blobs for d, _, _ in at], threads=8, frontiers=[wire.encode_frontiers(fr) for _, fr, _ in at])
    for (d, fr, upd), g in zip(at, got):
        assert g == d.model.result(fr), (d.label, fr, g, d.model.result(fr))
        if upd is not None:       # updates that hold exactly this version: the oracle's ids of it
            for cid in d.model.sequences():
                assert _oracle.visible_ids([upd], cid, cid.kind) == d.model.visible_ids(cid, fr), (d.label, fr, cid)
    assert len(at) >= 3 * len(docs)


# ------------------------------------------------------------------------------------------- (c) the model against the kernel-logic harness
CONFIGS = [{"LM_SPAN": "1"}, {"LM_SPAN": "1", "LM_PLAIN": "0"}, {"LM_SPAN": "1", "LM_PLAIN": "1"}, {"LM_SPAN": "0"}]
CONFIGS = CONFIGS + [dict(c, LM_CUT_MIN_ROWS="0") for c in CONFIGS]


def entries(docs, checkouts, n_versions=2):
    """(labels, blobs, frontiers, the model's results) of the documents at the latest version and, with `checkouts`, at their versions"""
    at = [(d, None) for d in docs] + ([(d, fr) for d in docs for fr in d.versions[:n_versions]] if checkouts else [])
    return ([(d.label, fr) for d, fr in at], [d.blobs for d, _ in at], [None if fr is None else wire.encode_frontiers(fr) for _, fr in at],
            [d.model.result(fr) for d, fr in at])


def compare(got, labels, blobs, fronts, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            third = _oracle.merge(blobs[i], frontiers=fronts[i])
            raise AssertionError("%s %s:\n kernel %r\n model  %r\n oracle %r" % (what, labels[i], g[:3], w[:3], third[:3]))
    assert len(got) == len(want)


@pytest.mark.parametrize("env", CONFIGS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_model_against_harness(corpora, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    docs = [d for ds in corpora.values() for d in ds]
    labels, blobs, fronts, want = entries(docs, "LM_PLAIN" not in env, n_versions=1)
    compare(_emu.merge_batch(blobs, fronts), labels, blobs, fronts, want, env)


def test_hand_built_documents(monkeypatch):
    """the documents of tests/test_gpu_zz_merge_ref.py through the harness (and the oracle), under the knobs that module uses"""
    three = [_merge_docs.three_peer_text(n, n) for n in (70, 130, 300)]
    sweep, windows, back = _merge_docs.sweep_docs(), _merge_docs.id_window_docs(), _merge_docs.backspace_docs()
    groups = [(three, {}), (three, {"LM_DIR_OPT_MAX": "4"}), (sweep[::3], {"LM_PLAIN": "2"}), (sweep[1::3], {"LM_PLAIN": "0"}),
              (_merge_docs.linear_prefix_docs(), {"LM_CUT_MIN_ROWS": "0"}), (windows, {}), (windows, {"LM_SPAN": "0"}),
              (back, {}), (back, {"LM_SPAN": "0"}), (back, {"LM_PLAIN": "0"})]
    for docs, env in groups:
        labels, blobs, fronts, want = entries(docs, True)
        compare(_oracle.merge_batch(blobs, frontiers=fronts, threads=8), labels, blobs, fronts, want, "oracle")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with Context(_emu.binding()) as c:
            compare(c.merge_batch(blobs, fronts), labels, blobs, fronts, want, env)
            assert "LM_DIR_OPT_MAX" not in env or c.sizing()[3] >= 1
        for k in env:
            monkeypatch.delenv(k)


# ------------------------------------------------------------------------------------------- (d) lm_delta / lm_cursor_pos expectations from the model
def test_lm_delta_with_ids_from_the_model():
    docs, pairs = _delta.fuzz_corpus(range(600, 612), n_steps=80, model=True)
    _delta.fuzz_condition(pairs)
    with Context(_emu.binding()) as c:
        assert _delta.run_fuzz(c, docs, pairs, "ids from the model") > 12 * 4


def test_lm_cursor_pos_with_ids_from_the_model():
    docs, pq, pw, aq, aw = _cursor.fuzz_corpus(range(600, 612), model=True)
    assert sum(1 for w in pw if w[0] == _cursor.DELETED) >= 12 * 2 * 11 and sum(1 for w in pw if w[0] == _cursor.NOT_FOUND) >= 12 * 2 * 5
    with Context(_emu.binding()) as c:
        res = c.merge_batch(docs)
        assert res == _oracle.merge_batch(docs)
        assert _cursor.check(c, pq, pw, aq, aw, "ids from the model") > 4000
        assert c.fetch() == res
