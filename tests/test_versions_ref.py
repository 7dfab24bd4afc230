"""lm_frontiers / lm_versions (k_version, Engine::versions) through the kernel-logic harness against the statement over the plain merge
model (tests/_versions_ref.py): the hand literals first, then the corpus — every recorded version all five ways — the hand-built
documents on the kernel's boundaries, and the batch shapes.  The floors (module docstring of _versions_ref.py) are asserted from the
statement before anything is compared.

Time: 20 to 30 s for the module in one process (22 tests; 9 s more where the snapshot test has to build the oracle first)."""
import json
import os

import pytest

import _emu, _versions_ref as R
import _import_lca as IL
from loro_amd import wire
from loro_amd._cabi import Context

SETTINGS = [None, ("LM_CUT_MIN_ROWS", "0"), ("LM_SPAN", "0"), ("LM_DECODE", "0")]
IDS = ["default", "LM_CUT_MIN_ROWS=0", "LM_SPAN=0", "LM_DECODE=0"]


def test_the_statement_gives_the_hand_written_answers():
    d, lit = R.hand_literals()
    for q, w in lit:
        assert R.answer(d.ref, q) == w, (q[1], [x.hex() for x in q[2:]], R.answer(d.ref, q), w)
    assert len(lit) == 34
    docs, qs = R.hand_docs()
    assert R.check_literals_against_the_statement(docs, qs) > 800


@pytest.fixture(scope="module")
def corp():
    docs = R.corpus()
    qs = [x for k, d in enumerate(docs) for x in R.version_queries(k, d)]
    tot = R.counts(docs, qs)
    print(len(qs), tot)
    R.check_floors(tot)
    return docs, qs


@pytest.fixture(scope="module")
def hand():
    return R.hand_docs()


def test_hand_literals_on_the_device():
    d, lit = R.hand_literals()
    with Context(_emu.binding()) as c:
        assert R.run_latest(c, [d], lit, "literals") == 34


@pytest.mark.parametrize("env", SETTINGS, ids=IDS)
def test_hand_built_documents(hand, monkeypatch, env):
    if env:
        monkeypatch.setenv(*env)
    docs, qs = hand
    with Context(_emu.binding()) as c:
        assert R.run_latest(c, docs, qs, str(env)) > 800


@pytest.mark.parametrize("env", SETTINGS, ids=IDS)
def test_every_version_of_the_corpus_all_five_ways(corp, monkeypatch, env):
    if env:
        monkeypatch.setenv(*env)
    docs, qs = corp
    with Context(_emu.binding()) as c:
        assert R.run_latest(c, docs, qs, str(env)) > 5000


def test_round_trips_on_every_version(corp):
    """TO_FRONTIERS(TO_VV(f)) == heads(f); TO_VV(TO_FRONTIERS(v)) == v for closed v — through the device both ways"""
    docs, _ = corp
    with Context(_emu.binding()) as c:
        c.merge_batch([d.blobs for d in docs])
        first = [(k, R.TO_VV, R.enc_frontiers(F)) for k, d in enumerate(docs) for F in d.versions]
        vvs = c.versions(first)
        back = c.versions([(q[0], R.TO_FRONTIERS, g[2]) for q, g in zip(first, vvs)])
        again = c.versions([(q[0], R.TO_VV, g[2]) for q, g in zip(first, back)])
        at = 0
        for k, d in enumerate(docs):
            for F in d.versions:
                assert vvs[at][0] == 0 and back[at] == (0, 0, R.enc_frontiers(d.ref.heads(F))), (d.label, F)
                assert again[at] == vvs[at], (d.label, F)
                at += 1
        assert at > 500


def test_one_call_of_many_queries_shuffled_across_documents_and_ops(corp, hand):
    """the host's grouping and the scatter back: every answer at its own index; 0 queries; lm_fetch the same before and after"""
    docs = corp[0] + hand[0]
    qs = corp[1] + [((q[0] + len(corp[0]),) + q[1:], w) for q, w in hand[1]]
    with Context(_emu.binding()) as c:
        res = c.merge_batch([d.blobs for d in docs])
        assert c.versions([]) == []
        assert R.check(c, R.shuffled(qs), "shuffled") > 8000
        assert c.fetch() == res


def test_checkouts_batch_entries_and_a_folded_document(corp):
    """a checkout of lm_frontiers(doc, 0) renders the latest bytes; for a checkout entry lm_frontiers(doc, 1) == heads(given) and
    TO_VV(given) == the entry's fetched vv; three checkouts of ONE document fold (shared replay) and answer per entry"""
    docs = corp[0][:8]
    with Context(_emu.binding()) as c:
        c.merge_batch([d.blobs for d in docs])
        heads = [c.frontiers(k, 0) for k in range(len(docs))]
        blobs, fronts, given, owner = [], [], [], []
        for k, d in enumerate(docs):
            blobs.append(d.blobs); fronts.append(heads[k]); given.append(None); owner.append(k)
            for F in d.versions[:3]:
                blobs.append(d.blobs); fronts.append(wire.encode_frontiers(F)); given.append(F); owner.append(k)
        # (entries that share one list object of blobs: what lm_stage folds)
        res = c.merge_batch(blobs, fronts)
        assert c.b.shared_documents(c.h) > 0
        qs = []
        for i, (k, F) in enumerate(zip(owner, given)):
            d = docs[k]
            if F is None:
                assert res[i] == d.model.result(), d.label
            else:
                assert res[i] == d.model.result(F), (d.label, F)
                qs.append(((i, R.TO_VV, R.enc_frontiers(F)), (0, 0, res[i][2])))
        assert R.check(c, qs, "TO_VV(given) == the fetched vv") == 24
        for i, (k, F) in enumerate(zip(owner, given)):
            R.check_heads(c, i, docs[k], F, "folded")
        # the applied history is the whole document's for every entry: a version beyond the checkout converts
        all_q = [((i,) + q[0][1:], q[1]) for i, k in enumerate(owner) if given[i] is not None for q in R.version_queries(k, docs[k])[:40]]
        R.check(c, all_q, "entries at a checkout")
        assert c.fetch() == res


@pytest.mark.parametrize("env", [None, ("LM_SHARE_REPLAY", "0"), ("LM_SPAN", "0")], ids=["default", "LM_SHARE_REPLAY=0", "LM_SPAN=0"])
def test_one_batch_of_entries_with_and_without_a_checkout(corp, monkeypatch, env):
    """folded by default (every entry a resident document once the first call has unfolded the batch); with LM_SHARE_REPLAY=0 / LM_SPAN=0 plain batch entries of both kinds side by side"""
    if env:
        monkeypatch.setenv(*env)
    with Context(_emu.binding()) as c:
        assert R.run_mixed(c, corp[0][:10], str(env)) > 1000


def test_the_recipe_for_diff_a_b(corp):
    """LoroDoc::diff(a, b): check out b, TO_VV(a), lm_delta — equals lm_delta from the model's vector for a"""
    docs = [d for d in corp[0] if len(d.versions) >= 4][:4]
    pairs = []
    for d in docs:
        big = max(d.versions, key=lambda F: len(d.ref.closure(F)))
        small = [F for F in d.versions if d.ref.closure(F) < d.ref.closure(big)][:3]
        pairs.append((big, small))
    with Context(_emu.binding()) as c:
        c.merge_batch([d.blobs for d in docs], [wire.encode_frontiers(b) for b, _ in pairs])
        qs = [(k, a) for k, (_, small) in enumerate(pairs) for a in small]
        assert len(qs) >= 6
        vvs = c.versions([(k, R.TO_VV, R.enc_frontiers(a)) for k, a in qs])
        assert all(v[0] == 0 for v in vvs)
        got = c.delta([(k, v[2]) for (k, a), v in zip(qs, vvs)])
        want = c.delta([(k, docs[k].model.vv(a)) for k, a in qs])
        assert got == want and all(g[0] == 0 for g in got)
        assert [v[2] for v in vvs] == [docs[k].model.vv(a) for k, a in qs]


def test_resident_documents_after_every_step_and_a_failed_step():
    """the six-step sessions of _import_lca.corpus (every fifth with a damaged blob: the step fails and is delivered again): after every
    step that goes through the heads are those of the applied set, ids of pending changes are refused; after a failed step the
    document stands where it stood before and so do its heads (both ways), unchanged there — before its first step that goes
    through: the empty version — and they move on with the next step that goes through"""
    docs = IL.corpus({"flat": 15, "text": 10, "movable": 5})
    sessions = [d.wire_steps() for d in docs]
    n_failed = n_pending = n = n_moved_on = 0
    stood = [R.enc_frontiers([])] * len(docs)          # the heads after the document's last step that went through
    after_failed = [False] * len(docs)
    with Context(_emu.binding()) as c:
        for k in range(IL.N_STEPS):
            blobs = [s[k][0] for s in sessions]
            if k == 0:
                c.stage(blobs, None); c.import_more([[] for _ in blobs], None)
            else:
                c.import_more(blobs, None)
            c.run()
            res = c.fetch()
            qs = []
            for i, d in enumerate(docs):
                f = d.facts()[k]
                if f.failed:
                    n_failed += 1
                    assert res[i][0] not in (0, 4, 6), (d.label, k)
                    assert c.frontiers(i, 0) == stood[i] and c.frontiers(i, 1) == stood[i], (d.label, k, c.frontiers(i, 0), stood[i])
                    after_failed[i] = True
                    continue
                ref = R.Ref(f.model)
                want = R.enc_frontiers(ref.doc_heads())
                assert c.frontiers(i, 0) == want and c.frontiers(i, 1) == want, (d.label, k)
                n_moved_on += after_failed[i] and want != stood[i]
                after_failed[i] = False
                stood[i] = want
                H = ref.doc_heads()
                qs.append(((i, R.CMP_DOC, want), (0, R.EQUAL, b"")))
                qs.append(((i, R.TO_VV, want), (0, 0, res[i][2])))
                qs.append(((i, R.TO_FRONTIERS, res[i][2]), (0, 0, want)))
                if H:
                    qs.append(((i, R.MINIMIZE, R.enc_frontiers(H + sorted(ref.closure(H))[:3])), (0, 0, want)))
                delivered = {(ch.peer, x) for s in d.steps[:k + 1] if not s[2] for _, cs in s[0] for ch in cs for x in range(ch.counter, ch.ctr_end)}
                pend = sorted(delivered - f.model.all_ids)
                if pend:
                    n_pending += 1
                    qs.append(((i, R.TO_VV, R.enc_frontiers(pend[:1])), (R.NOT_FOUND, 0, b"")))
                    qs.append(((i, R.CMP_DOC, R.enc_frontiers(pend[:1])), (0, R.LESS, b"")))
            n += R.check(c, qs, "step %d" % k)
            assert c.fetch() == res
    assert n_failed >= 5 and n_moved_on >= 5 and n_pending >= 20 and n > 500, (n_failed, n_moved_on, n_pending, n)


def test_a_snapshot_staged_document_a_shallow_snapshot_and_a_damaged_document(corp):
    import _oracle
    d = corp[0][1]
    full = wire.Replica(1)
    reps_changes = {}
    for ch in d.changes:
        reps_changes.setdefault(ch.peer, []).append(ch)
    full.changes = {p: sorted(cs, key=lambda x: x.counter) for p, cs in reps_changes.items()}
    full.vv = dict(d.ref.end)
    full.frontiers = d.ref.doc_heads()
    st, ents = _oracle.state_entries([full.export()])
    assert st == 0
    snap = full.export_snapshot(state=ents)
    shallow = wire.envelope(b"\x00" * 8 + b"\x01\x00\x00\x00" + b"E", mode=3)
    bad = bytearray(d.blobs[0]); bad[-1] ^= 1
    qs = [x for x in R.version_queries(0, d)]
    with Context(_emu.binding()) as c:
        res = c.merge_batch([[snap], [shallow], [bytes(bad)]])
        assert c.b.state_documents(c.h) == 1 and res[0] == d.model.result()
        assert res[1][0] == R.UNSUPPORTED and res[2][0] not in (0, 4, 6)
        R.check_heads(c, 0, d, None, "snapshot")
        R.check(c, qs, "snapshot")
        assert c.frontiers(1, 0) is None and c.frontiers(2, 1) is None
        z = bytes([0])
        assert c.versions([(1, R.TO_VV, z), (2, R.CMP_DOC, z), (1, R.TO_VV, b""), (2, R.CMP, z, z)]) == \
            [(R.UNSUPPORTED, 0, b""), (res[2][0], 0, b""), (R.UNSUPPORTED, 0, b""), (res[2][0], 0, b"")]
        assert c.fetch() == res


def test_a_fused_map_batch_and_documents_replayed_in_the_side_engine(corp, hand, monkeypatch):
    """LWW Map documents decoded without op rows (k_map_fused): the DAG stage runs for them too — the hand-built documents are Map
    documents and stay on that path; the corpus's Map sessions (values the fused decoder leaves to the row decoders) are flagged there
    and replayed in the side engine, which answers for them"""
    monkeypatch.setenv("LM_MF_MIN_ROWS", "1"); monkeypatch.setenv("LM_MF_CHG_RATIO", "0")
    docs, qs = hand
    with Context(_emu.binding()) as c:
        assert R.run_latest(c, docs, qs, "fused") > 800
        # (the 20,000-row document is beyond what the fused decoder takes: handed over, and answered in the side engine)
        assert (c.b.fused_documents(c.h), c.b.redo_documents(c.h)) == (len(docs), 1)
    docs = [d for d in corp[0] if all(o.cid.kind == wire.KIND_MAP for ch in d.changes for o in ch.ops)]
    assert len(docs) == 10
    qs = [x for k, d in enumerate(docs) for x in R.version_queries(k, d)]
    with Context(_emu.binding()) as c:
        assert R.run_latest(c, docs, qs, "side engine") > 1000
        assert (c.b.fused_documents(c.h), c.b.redo_documents(c.h)) == (len(docs), len(docs))


def test_a_soft_unsupported_fixture_answers_normally():
    """a document of the reference that holds Tree / Counter containers beside the rest: LM_UNSUPPORTED with a rendering"""
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures.json")))["blobs"]
    blob = bytes.fromhex(fx["runtime-updates.ts.blob"])
    with Context(_emu.binding()) as c:
        res = c.merge_batch([[blob]])
        assert res[0][0] == R.UNSUPPORTED and res[0][1]
        heads = c.frontiers(0, 0)
        assert heads is not None and c.frontiers(0, 1) == heads
        got = c.versions([(0, R.TO_VV, heads), (0, R.TO_FRONTIERS, res[0][2]), (0, R.CMP_DOC, heads), (0, R.MINIMIZE, heads)])
        assert got == [(0, 0, res[0][2]), (0, 0, heads), (0, R.EQUAL, b""), (0, 0, heads)]


def test_the_calls_that_cannot_be_answered():
    import ctypes
    a = wire.Replica(7); a.text_insert("text", 0, "hello"); a.commit()
    z = bytes([0])
    with Context(_emu.binding()) as c:
        c.stage([[a.export()]])
        with pytest.raises(RuntimeError, match="before lm_run"):
            c.versions([(0, R.TO_VV, z)])
        assert c.frontiers(0, 0) is None
        c.run()
        with pytest.raises(RuntimeError, match="no such document"):
            c.versions([(1, R.TO_VV, z)])
        with pytest.raises(RuntimeError, match="LM_VER"):
            c.versions([(0, 5, z)])
        with pytest.raises(RuntimeError, match="LM_VER"):
            c.versions([(0, -1, z)])
        assert c.frontiers(1, 0) is None and c.frontiers(0, 2) is None
        want = R.enc_frontiers([(7, 4)])
        buf = ctypes.create_string_buffer(64)
        assert c.b.frontiers(c.h, 0, 0, buf, len(want)) == len(want) and buf.raw[:len(want)] == want
        assert c.b.frontiers(c.h, 0, 0, buf, len(want) - 1) == -1
        assert c.versions([(0, R.TO_VV, want)]) == [(0, 0, R.enc_vv({7: 5}))]
        c.import_more([[]], None)
        with pytest.raises(RuntimeError, match="before lm_run"):
            c.versions([(0, R.TO_VV, z)])
        c.run()
        c.run_async()                                    # a run in flight: -1 for both calls, then the answers again
        try:
            with pytest.raises(RuntimeError, match="in flight"):
                c.versions([(0, R.TO_VV, z)])
            assert c.frontiers(0, 0) is None
        finally:
            c.wait()
        assert c.frontiers(0, 0) == want and c.versions([(0, R.TO_VV, want)]) == [(0, 0, R.enc_vv({7: 5}))]
