"""lm_cursor_pos / lm_cursor_at (k_cursor, Engine::cursor) through the kernel-logic harness against the cursor rules restated over
the plain merge model (tests/_cursor_ref.py): styled Text, child containers, any version, documents that arrive in steps, and
documents built on the kernel's own boundaries.  The expectation is the model's alone: every run's (status, JSON, version vector,
pending) must equal the model's before a cursor is asked; the oracle only writes the state bytes of the snapshot test.

Floors, asserted from the model before anything is compared (count seen):
  rich (24 sessions, 3 peers, styles="rich", text / text + list; every id of `order`, the extras of _cursor.container_queries, every
  position: 8,774 + 5,915 queries at the latest version): answers with pos != entity index >= 200 (5,613); cursors that ARE
  anchors >= 50 (231); DELETED with an anchor in front >= 50 (1,477); pos16 != pos >= 50 (5,565; the writers' alphabet holds
  U+1F600 already, _fuzz.py is unchanged); containers of more than 64 entities >= 20 (35); of more than 64 id-contiguous runs of one
  visibility — a lower bound of the items, so more than one leaf — >= 20 (36).
  nested (24 sessions, 386 sequence containers, 362 of them children of Map / List, all asked in one call): DELETED in children >= 50
  (504).
  versions (rich + nested, 1,247 entries: the latest, every recorded frontier, a change end, a version inside a change, two concurrent
  heads; 48 entries have more than one head, >= 20 asked): ids V lacks with elements of another peer that V holds within eight places
  on both sides >= 200 (38,027); ids visible at V and deleted later >= 100 (19,010); DELETED at V >= 100 (33,206).  Each version runs
  as a batch entry with LM_SHARE_REPLAY=1 and =0 and on resident documents (lm_stage + lm_run, then an lm_import that brings nothing).
  steps (30 six-step sessions of _merge_docs_steps + its 18 new-peer documents): steps with pending atoms, whose ids are asked and
  must be ID_NOT_FOUND, >= 20 (109); steps that bring a peer sorting in front of a stored one >= 20 (43).  Both versions a step
  stands at are asked.
Boundary documents (_cursor_ref.boundary_docs, 75 documents, 14,757 + 11,674 queries, then the same in ONE shuffled call — the host's
sort and scatter; the window documents assert from the model that their astral scalar / tombstone stands at the entity index they
name), literals for a child whose Map key is overwritten, a child without an op, containers in front of their first op, 65 roots.
Settings: everything under the default; under LM_SPAN=0 (batch forms only), LM_CUT_MIN_ROWS=0 and LM_DIR_OPT_MAX=4 the latest corpora,
the boundary documents, the steps, and EVERY version (155 entries) of a smaller corpus of four styled and four nested sessions, three
ways (_cursor_ref.small_version_docs; the floors are asserted on the large corpus, which runs under the default).

Time: 370 s for the module in one process on an 8-thread host (the versions three ways 265 s, the three other settings 75 s).
"""
import pytest

import _cursor_ref as R, _emu
from _cursor import DELETED, LEFT, MIDDLE, RIGHT
from loro_amd import wire
from loro_amd._cabi import Context


def test_the_restatement_gives_the_hand_written_answers():
    """before anything else: every literal of _cursor.hand_cases(), written out by hand from the reference, from the rules alone"""
    n = 0
    for name, model, pq, pw, aq, aw in R.hand_models():
        gw, ga = R.model_answers(model, pq, aq)
        assert gw == pw, (name, [(q, g, w) for q, g, w in zip(pq, gw, pw) if g != w])
        assert ga == aw, (name, [(q, g, w) for q, g, w in zip(aq, ga, aw) if g != w])
        n += len(pw) + len(aw)
    assert n == 53


@pytest.fixture(scope="module")
def rich():
    docs = R.rich_docs(R.RICH_SEEDS)
    e = R.entries(docs)
    R.check_floors("rich", R.count(e[6], e[2], e[3]), R.RICH_FLOORS)
    return docs, e


@pytest.fixture(scope="module")
def nested():
    docs = R.nested_docs(R.NESTED_SEEDS)
    e = R.entries(docs)
    kids = sum(1 for q, w in zip(e[2], e[3]) if w[0] == DELETED and not q[1].startswith("cid:root-"))
    assert kids >= R.NESTED_FLOORS["deleted_in_children"], kids
    return docs, e


def run_batch(e, what):
    blobs, fronts, pq, pw, aq, aw, _, want = e
    with Context(_emu.binding()) as c:
        res = c.merge_batch(blobs, fronts)
        assert res == want, what
        n = R.check(c, pq, pw, aq, aw, what)
        assert c.fetch() == res
    return n


def test_rich_documents_at_the_latest_version(rich):
    assert run_batch(rich[1], "rich") > 15000


def test_nested_documents_every_sequence_container_in_one_call(nested):
    assert run_batch(nested[1], "nested") > 15000


def test_documents_that_arrive_in_steps_at_both_versions_of_every_step():
    docs = R.step_docs()
    R.check_floors("steps", R.step_counts(docs), R.STEP_FLOORS)
    with Context(_emu.binding()) as c:
        assert R.run_steps(c, docs) > 10000


# ------------------------------------------------------------------------------------------------------------------------ versions
@pytest.fixture(scope="module")
def versions(rich, nested):
    docs = rich[0] + nested[0]
    R.check_floors("versions", R.version_counts(docs), R.VERSION_FLOORS)
    assert sum(1 for d in docs for _, fr in d.versions if fr is not None and len(fr) > 1) >= 20       # multi-head frontiers
    return docs


@pytest.mark.parametrize("share", ["1", "0"])
def test_every_version_as_a_batch_entry(versions, monkeypatch, share):
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    assert run_batch(R.entries(versions, "all"), "versions, LM_SHARE_REPLAY=" + share) > 100000


def test_every_version_of_resident_documents(versions):
    with Context(_emu.binding()) as c:
        assert R.run_resident_versions(c, versions) > 100000


# ---------------------------------------------------------------------------------------------------------------------- boundaries
@pytest.fixture(scope="module")
def boundary():
    docs = R.boundary_docs()
    return docs, R.entries(docs)


def run_boundary(boundary, what):
    docs, e = boundary
    blobs, fronts, pq, pw, aq, aw, _, want = e
    with Context(_emu.binding()) as c:
        res = c.merge_batch(blobs, fronts)
        assert res == want, what
        n = R.check(c, pq, pw, aq, aw, what)
        for k, d in enumerate(docs):
            if d.label in ("one peer", "two peers", "255 peers"):
                q, w = R.peer_queries(k, d)
                n += R.check(c, q, w, [], [], what + ", ids no element has")
            if d.label in ("three leaves", "a hole of leaves and a deleted tail"):
                for q, w in R.chunk_queries(k, d):
                    n += R.check(c, q, w, [], [], what + ", %d queries" % len(q))
        n += R.check(c, *R.shuffled(pq, pw, aq, aw), what + ", shuffled")       # the host's sort and its scatter
        assert c.fetch() == res
    return n


def test_documents_on_the_kernels_boundaries(boundary):
    assert run_boundary(boundary, "boundaries") > 50000


def test_a_child_whose_parent_entry_is_overwritten_and_a_child_without_an_op():
    d, pq, pw, aq, aw, ekey = R.unreachable_child_case()
    with Context(_emu.binding()) as c:
        res = c.merge_batch([d.blobs])
        assert res == [d.model.result()]
        R.check(c, pq, pw, aq, aw, "unreachable child")
        # A child that never received an op: the device's container table lists the containers an op ADDRESSES, so the key names
        # nothing there — a refusal, pinned.  The reference knows the container from its parent's value (has_container,
        # loro.rs:1135-1142) and would answer IdNotFound for the id (loro.rs:1911-1917) and length 0 without one (:1980-1996).
        assert c.cursor_pos([(0, ekey, (5, 1), MIDDLE), (0, ekey, None, RIGHT)]) == [(R.NO_CONTAINER, 0, 0, MIDDLE), (R.NO_CONTAINER, 0, 0, RIGHT)]
        assert c.cursor_at([(0, ekey, 0, MIDDLE)]) == [(R.NO_CONTAINER, None, MIDDLE, 0)]
        # a key whose peer does not fit 64 bits names nothing (2^64 - 1 does: "children (p, 0) of six peers")
        assert c.cursor_pos([(0, "cid:0@18446744073709551616:Text", None, RIGHT)]) == [(R.NO_CONTAINER, 0, 0, RIGHT)]


def run_empty_container_batch(what):
    d, fr, pq, pw, aq, aw = R.empty_container_case()
    exs = {x.key: x for x in (R.Expect(d.model, c, fr) for c in R.sequence_cids(d.model))}
    assert [exs[q[1]].pos_answer(q[2], q[3]) for q in pq] == pw and [exs[q[1]].at_answer(q[2], q[3]) for q in aq] == aw      # the rules give the literals
    with Context(_emu.binding()) as c:
        res = c.merge_batch([d.blobs, d.blobs], [wire.encode_frontiers(fr), None])
        assert res == [d.model.result(fr), d.model.result()], what
        R.check(c, pq, pw, aq, aw, what)


@pytest.mark.parametrize("share", ["1", "0"])
def test_a_container_in_front_of_its_first_op(monkeypatch, share):
    """an entry checked out in front of the first op of a Text and of a List (literals): one leaf, nothing in it — `nr == 0` itself is
    unreachable (_cursor_ref.empty_container_case); then the same version on a resident document, whose leaves hold future elements"""
    monkeypatch.setenv("LM_SHARE_REPLAY", share)
    run_empty_container_batch("empty containers, LM_SHARE_REPLAY=" + share)
    d, fr, pq, pw, aq, aw = R.empty_container_case()
    with Context(_emu.binding()) as c:
        c.stage([d.blobs]); c.run()
        c.import_more([[]], [wire.encode_frontiers(fr)]); c.run()
        R.check(c, pq, pw, aq, aw, "empty containers, resident")


def test_a_document_beyond_the_root_limit_is_refused_not_guessed():
    d = R.too_many_roots_doc()
    with Context(_emu.binding()) as c:
        res = c.merge_batch([d.blobs])
        assert res[0][0] == 4                                                    # LM_UNSUPPORTED
        assert c.cursor_pos([(0, "cid:root-t000:Text", (69, 0), MIDDLE), (0, "cid:root-t064:Text", None, RIGHT)]) == [(R.UNSUPPORTED, 0, 0, MIDDLE), (R.UNSUPPORTED, 0, 0, RIGHT)]
        assert c.cursor_at([(0, "cid:root-t000:Text", 0, LEFT)]) == [(R.UNSUPPORTED, None, LEFT, 0)]


# ------------------------------------------------------------------------------------------------------------------------ settings
SETTINGS = [("LM_SPAN", "0"), ("LM_CUT_MIN_ROWS", "0"), ("LM_DIR_OPT_MAX", "4")]


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: "%s=%s" % e)
def test_corpora_and_boundaries_under_other_settings(rich, nested, boundary, monkeypatch, env):
    """everything above once more; the versions are those of a smaller corpus (_cursor_ref.small_version_docs), all of them, as batch
    entries both ways and — but for LM_SPAN=0: resident documents are span-granular — on resident documents"""
    monkeypatch.setenv(*env)
    what = "%s=%s" % env
    run_batch(rich[1], "rich, " + what)
    run_batch(nested[1], "nested, " + what)
    run_boundary(boundary, "boundaries, " + what)
    small = R.small_version_docs()                 # every version of these, three ways
    for share in ("1", "0"):
        monkeypatch.setenv("LM_SHARE_REPLAY", share)
        run_batch(R.entries(small, "all"), "versions, %s, LM_SHARE_REPLAY=%s" % (what, share))
        run_empty_container_batch("empty containers, %s, LM_SHARE_REPLAY=%s" % (what, share))
    monkeypatch.delenv("LM_SHARE_REPLAY")
    if env[0] != "LM_SPAN":
        with Context(_emu.binding()) as c:
            R.run_resident_versions(c, small, "resident, " + what)
        with Context(_emu.binding()) as c:
            R.run_steps(c, R.step_docs(), "steps, " + what)


def test_state_staged_snapshots_of_ten_rich_documents(rich):
    """a document that is ONE snapshot is staged from its state section (no element ids there): the first cursor call stages it
    through its history.  The state section's bytes are the oracle's state writer's, the expectation is the model's"""
    import _oracle
    docs = rich[0][:10]
    snaps = []
    for d in docs:
        full = wire.Replica(d.reps[0].peer)
        for r in d.reps:
            full.merge_from(r)
        st, ents = _oracle.state_entries([full.export()])
        assert st == 0
        snaps.append([full.export_snapshot(state=ents)])
    _, _, pq, pw, aq, aw, _, want = R.entries(docs)
    with Context(_emu.binding()) as c:
        res = c.merge_batch(snaps)
        assert c.b.state_documents(c.h) == 10 and [r[:2] for r in res] == [w[:2] for w in want]
        R.check(c, pq, pw, aq, aw, "state-staged snapshots")
        assert c.fetch() == res
