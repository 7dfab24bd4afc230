"""GPU parity for lm_frontiers / lm_versions against the statement over the plain merge model (tests/_versions_ref.py): k_version on
the device on the hand literals, the hand-built documents of test_versions_ref.py (peer counts on the lane strides, the edge peer ids,
the chain, the pending changes, malformed bytes) under the default, LM_CUT_MIN_ROWS=0, LM_SPAN=0 and LM_DECODE=0, and a third of the
corpus's versions in ONE batch of more than 256 documents (both streams).  The kernel-logic harness does not model inactive lanes in
permutes; the device does.  Every floor is asserted from the statement before anything runs.  Nothing here reads the reference tree.
"""
import pytest

import _versions_ref as R
from loro_amd import wire

pytestmark = pytest.mark.gpu

SETTINGS = [None, ("LM_CUT_MIN_ROWS", "0"), ("LM_SPAN", "0"), ("LM_DECODE", "0")]
IDS = ["default", "LM_CUT_MIN_ROWS=0", "LM_SPAN=0", "LM_DECODE=0"]


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hand():
    docs, qs = R.hand_docs()
    assert R.check_literals_against_the_statement(docs, qs) > 800
    return docs, qs


@pytest.fixture(scope="module")
def corp():
    docs = R.corpus()
    every = [x for k, d in enumerate(docs) for x in R.version_queries(k, d)]
    R.check_floors(R.counts(docs, every))
    # a third of the versions, the documents nine times over: 270 documents, two streams
    reps = 9
    batch = docs * reps
    qs = []
    for r in range(reps):
        for k, d in enumerate(docs):
            i = r * len(docs) + k
            qs += [((i,) + q[1:], w, t) for j, (q, w, t) in enumerate(R.version_queries(k, d)) if j % 3 == r % 3]
    R.check_floors(R.counts(batch, qs))
    return batch, qs


def test_hand_literals(engine):
    d, lit = R.hand_literals()
    for q, w in lit:
        assert R.answer(d.ref, q) == w
    assert R.run_latest(engine, [d], lit, "literals") == 34


@pytest.mark.parametrize("env", SETTINGS, ids=IDS)
def test_hand_built_documents(engine, hand, monkeypatch, env):
    if env:
        monkeypatch.setenv(*env)
    docs, qs = hand
    assert R.run_latest(engine, docs, qs, str(env)) > 800


@pytest.mark.parametrize("env", SETTINGS, ids=IDS)
def test_a_third_of_the_corpus_in_one_batch_of_270_documents(engine, corp, monkeypatch, env):
    if env:
        monkeypatch.setenv(*env)
    docs, qs = corp
    assert len(docs) > 256
    assert R.run_latest(engine, docs, R.shuffled(qs), str(env)) > 20000
    assert engine.b.n_streams(engine.h) == 2


def test_checkout_entries_fold_and_answer_per_entry(engine, corp):
    docs = corp[0][:8]
    engine.merge_batch([d.blobs for d in docs])
    heads = [engine.frontiers(k, 0) for k in range(len(docs))]
    blobs, fronts, given, owner = [], [], [], []
    for k, d in enumerate(docs):
        blobs.append(d.blobs); fronts.append(heads[k]); given.append(None); owner.append(k)
        for F in d.versions[:3]:
            blobs.append(d.blobs); fronts.append(wire.encode_frontiers(F)); given.append(F); owner.append(k)
    res = engine.merge_batch(blobs, fronts)
    assert engine.b.shared_documents(engine.h) > 0
    qs = []
    for i, (k, F) in enumerate(zip(owner, given)):
        assert res[i] == docs[k].model.result(F), (docs[k].label, F)
        if F is not None:
            qs.append(((i, R.TO_VV, R.enc_frontiers(F)), (0, 0, res[i][2])))
    assert R.check(engine, qs, "TO_VV(given) == the fetched vv") == 24
    for i, (k, F) in enumerate(zip(owner, given)):
        R.check_heads(engine, i, docs[k], F, "folded")
    assert engine.fetch() == res


@pytest.mark.parametrize("env", [None, ("LM_SHARE_REPLAY", "0"), ("LM_SPAN", "0")], ids=["default", "LM_SHARE_REPLAY=0", "LM_SPAN=0"])
def test_one_batch_of_entries_with_and_without_a_checkout(engine, corp, monkeypatch, env):
    if env:
        monkeypatch.setenv(*env)
    assert R.run_mixed(engine, corp[0][:10], str(env)) > 1000


def test_resident_documents_in_steps_and_what_cannot_be_answered(engine):
    a, b = wire.Replica(7), wire.Replica(3)
    a.text_insert("text", 0, "hello"); a.commit()
    first = a.export()
    b.merge_from(a); b.set_visible("text", wire.KIND_TEXT, [(7, i) for i in range(5)])
    b.text_insert("text", 5, "!!"); b.commit()
    a.text_insert("text", 0, ">"); a.commit()
    own_b = wire.Replica(3); own_b.changes = {3: b.changes[3]}
    second = [own_b.export(), a.export({7: 5})]
    z = bytes([0])
    engine.stage([[first]])
    with pytest.raises(RuntimeError, match="before lm_run"):
        engine.versions([(0, R.TO_VV, z)])
    engine.run()
    assert engine.frontiers(0, 0) == R.enc_frontiers([(7, 4)])
    damaged = bytearray(second[0]); damaged[-1] ^= 1
    res = engine.step([[bytes(damaged)]])
    # a failed step: the document stands where it stood, and so do its heads
    assert res[0][0] not in (0, 4, 6) and engine.frontiers(0, 0) == R.enc_frontiers([(7, 4)]) and engine.frontiers(0, 1) == R.enc_frontiers([(7, 4)])
    res = engine.step([second], [R.enc_frontiers([(7, 4)])])
    assert res[0][0] == 0
    assert engine.frontiers(0, 0) == R.enc_frontiers([(3, 1), (7, 5)]) and engine.frontiers(0, 1) == R.enc_frontiers([(7, 4)])
    got = engine.versions([(0, R.TO_VV, R.enc_frontiers([(3, 1)])), (0, R.CMP, R.enc_frontiers([(3, 0)]), R.enc_frontiers([(7, 5)])),
                           (0, R.CMP_DOC, R.enc_frontiers([(7, 4)])), (0, R.TO_FRONTIERS, R.enc_vv({3: 2, 7: 6}))])
    assert got == [(0, 0, R.enc_vv({3: 2, 7: 5})), (0, R.CONCURRENT, b""), (0, R.GREATER, b""), (0, 0, R.enc_frontiers([(3, 1), (7, 5)]))]
    with pytest.raises(RuntimeError, match="no such document"):
        engine.versions([(1, R.TO_VV, z)])
    with pytest.raises(RuntimeError, match="LM_VER"):
        engine.versions([(0, 5, z)])
    assert engine.fetch() == res
