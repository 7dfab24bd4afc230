"""GPU parity for stable cursors (lm_cursor_pos / lm_cursor_at): k_cursor on the device through the C ABI against answers derived
from the oracle alone (_cursor.py).  The cases of the kernel-logic harness (test_emu_cursor.py) at larger sizes — the fiber harness
does not model inactive lanes in permutes or LDS apertures — plus configs[1]-shaped documents and a batch in which most documents
have no query."""
import random

import pytest

import _cursor, _fuzz, _oracle
from _cursor import OK, DELETED, NOT_FOUND, DOC_FAILED, LEFT, MIDDLE, RIGHT, TEXT, LIST
from loro_amd import wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


def test_hand_cases(engine):
    cases = _cursor.hand_cases()
    docs = [b for _, b, *_ in cases]
    docs.append([docs[0][0][:-2] + b"\x00\x01"])
    res = engine.merge_batch(docs)
    assert res == _oracle.merge_batch(docs) and res[-1][0] != 0
    pq, pw, aq, aw = [], [], [], []
    for d, (_, _, q, w, q2, w2) in enumerate(cases):
        pq += [(d,) + x[1:] for x in q]; pw += w; aq += [(d,) + x[1:] for x in q2]; aw += w2
    f = len(docs) - 1
    pq += [(f, TEXT, (7, 0), MIDDLE)]; pw += [(DOC_FAILED, 0, 0, MIDDLE)]
    aq += [(f, TEXT, 0, LEFT)]; aw += [(DOC_FAILED, None, LEFT, 0)]
    _cursor.check(engine, pq, pw, aq, aw, "hand")
    assert engine.fetch() == res


@pytest.mark.parametrize("env", [("LM_SPAN", "1"), ("LM_SPAN", "0"), ("LM_SPAN_AUTO", "1")])
def test_fuzz_documents_under_both_layouts_and_the_product_default(engine, monkeypatch, env):
    monkeypatch.setenv(*env)
    docs, pq, pw, aq, aw = _cursor.fuzz_corpus(range(200, 400), n_steps=110)
    res = engine.merge_batch(docs)
    assert res == _oracle.merge_batch(docs, threads=8)
    n = _cursor.check(engine, pq, pw, aq, aw, "%s=%s" % env)
    assert engine.fetch() == res
    assert n > 100000 and sum(1 for w in pw if w[0] == DELETED) > 5000


def test_a_long_chain_and_more_queries_than_one_pass_holds(engine):
    blobs = _cursor.chain_case(6000)
    ex = _cursor.Expect(blobs, blobs, "text", wire.KIND_TEXT)
    (pq, pw), (aq, aw) = _cursor.container_queries(0, TEXT, ex, random.Random(1))
    assert len(pq) > 5000 and sum(1 for w in pw if w[0] == DELETED) > 1000
    res = engine.merge_batch([blobs])
    assert res == _oracle.merge_batch([blobs])
    _cursor.check(engine, pq, pw, aq, aw, "chain")
    assert engine.fetch() == res


def test_config2_shaped_documents_at_the_latest_version_and_at_a_checkout(engine):
    """configs[1] of BASELINE.json: a 100k-op trace, 50k-op base + two concurrent 25k-op branches; the checkout is the end of the base"""
    from loro_amd import workload
    tpl = workload.Cfg2Template(50000, 25000, seed=0, commit_every=10, fuse=True)
    rng = random.Random(7)
    docs, fronts, pq, pw, aq, aw = [], [], [], [], [], []
    for d in range(2):
        blobs = tpl.stamp(d)
        latest = _cursor.Expect(blobs, blobs, "text", wire.KIND_TEXT)
        at_base = _cursor.Expect(blobs, blobs[:1], "text", wire.KIND_TEXT)
        (peer, end), = at_base.vv.items()
        for ex, fr in ((latest, None), (at_base, wire.encode_frontiers([(peer, end - 1)]))):
            q, w, q2, w2 = _cursor.sample_queries(len(docs), TEXT, ex, rng, 96)
            assert len(q) >= 64 and sum(1 for x in w if x[0] == DELETED) >= 8
            docs.append(blobs); fronts.append(fr); pq += q; pw += w; aq += q2; aw += w2
    assert sum(1 for w in pw if w[0] == NOT_FOUND) > 20      # ids the checkout leaves in the future among them
    res = engine.merge_batch(docs, fronts)
    assert [r[0] for r in res] == [0] * len(docs)
    _cursor.check(engine, pq, pw, aq, aw, "configs[1]")
    assert engine.fetch() == res


def test_resident_documents_across_an_import(engine):
    pairs = [_cursor.resident_pair(s) for s in range(48)]
    rng = random.Random(9)
    engine.stage([p[0] for p in pairs]); engine.run()
    for step, at in ((0, lambda p: p[0]), (1, lambda p: p[0] + p[1])):
        if step:
            engine.import_more([p[1] for p in pairs]); engine.run()
        res = engine.fetch()
        pq, pw, aq, aw = [], [], [], []
        for d, p in enumerate(pairs):
            ex = _cursor.Expect(p[0] + p[1], at(p), "text", wire.KIND_TEXT)
            (q, w), (q2, w2) = _cursor.container_queries(d, TEXT, ex, rng)
            pq += q; pw += w; aq += q2; aw += w2
        _cursor.check(engine, pq, pw, aq, aw, "resident step %d" % step)
        assert engine.fetch() == res


def test_a_large_batch_in_which_every_seventh_document_has_queries(engine):
    base = [_fuzz.blobs_of(_cursor.fuzz_session(500 + s)) for s in range(32)]
    exs = [(_cursor.Expect(b, b, "text", wire.KIND_TEXT), _cursor.Expect(b, b, "list", wire.KIND_LIST)) for b in base]
    docs = [base[i % 32] for i in range(2240)]
    rng = random.Random(11)
    pq, pw, aq, aw = [], [], [], []
    for d in range(0, len(docs), 7):
        et, el = exs[d % 32]
        for cid, ex in ((TEXT, et), (LIST, el)):
            q, w, q2, w2 = _cursor.sample_queries(d, cid, ex, rng, 24)
            pq += q; pw += w; aq += q2; aw += w2
    res = engine.merge_batch(docs)
    assert all(r[0] == 0 for r in res)
    _cursor.check(engine, pq, pw, aq, aw, "every 7th")
    assert engine.fetch() == res
