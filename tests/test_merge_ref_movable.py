"""The MovableList rules of the plain merge model (tests/_merge_ref.py: items placed by the sibling rule, a move as delete + insert
under one id, last_pos / last_value by (lamport, peer id), children by the creating op's id, the root rule) against
  (a) the reference's known answers the suite already holds, fed to the model from the same wire.Replica scripts: mov.rs:13-62,
      movable_list_state.rs:1940-2031, the script of the runtime fixture, test_emu_movable.existence_docs / nesting_docs;
  (b) the oracle: JSON bytes, version vector bytes and the alive item ids of every sequence container, at the latest version and at
      every recorded version, on corpora whose writers took their views from the MODEL, and on the hand-built documents;
  (c) the kernel-logic harness under the variants test_emu_movable.py uses: span, LM_SPAN=0, LM_DECODE=0 and LM_DIR_OPT_MAX=4.
Before anything is compared, every corpus must show each outcome of the sibling rule AND of the element rules often enough
(_merge_docs.check_conditions).  What the model does not cover stays with test_emu_movable.py: damaged rows, pending changes.

Time.  154 s for the module in one process on an 8-thread host (test_merge_ref.py: 129 s): the three corpora and their models 14.5 s
(the writers rebuild the model at every sync), the hand-built documents 3 s (the 1,500-element one 2.5 s), (a) 0.1 s, (b) 3.4 + 11.4 +
3.4 + 0.8 s, (c) the corpora 17 - 20 s per configuration (230 documents + 30 delivered as whole exports, and under LM_SPAN=1 / 0 two
checkouts of each: 260 or 780 runs) and the hand-built documents 7 - 9 s (19.5 s where LM_DIR_OPT_MAX=4 re-runs the large one).  Each
configuration is a test of its own, so pytest-xdist spreads them."""
import pytest

import _emu, _merge_docs, _merge_ref, _oracle
from _richtext_ref import changes_of
from loro_amd import wire
from loro_amd._cabi import Context
from test_merge_ref import compare, entries

ML = wire.KIND_MOVABLE
V = _merge_ref.view


def model_of(*reps):
    return _merge_ref.Model(changes_of(reps))


def take(dst, src, name="list"):
    """`dst` imports what `src` holds and looks at the list through the model"""
    src.commit()
    dst.merge_from(src)
    cid = wire.root_cid(name, ML)
    dst.set_visible(cid, ML, V(dst, cid))


@pytest.fixture(scope="module")
def corpora():
    out = _merge_docs.movable_corpora()
    for name, docs in out.items():
        _merge_docs.check_conditions(name, docs)
    return out


@pytest.fixture(scope="module")
def hand_built():
    """name -> [Doc]; the known values of the documents that have one are asserted here, on the model"""
    out = {"ties": _merge_docs.lamport_tie_docs(), "passes": _merge_docs.row_pass_docs(), "load": [_merge_docs.table_load_doc()]}
    out["delete"], want = _merge_docs.move_against_delete_docs()
    assert out["delete"][0].model.value() == {"ml": want[0]}
    assert "b" not in out["delete"][1].model.value()["ml"] and "b" in out["delete"][2].model.value()["ml"]
    split, at, want = _merge_docs.split_maxima_docs()
    for name, value in want.items():
        assert split.model.value(at.get(name)) == {"ml": value}, name
    out["split"] = [split]
    out["children"], want = _merge_docs.children_docs()
    assert [d.model.value() for d in out["children"]] == [{"ml": w} for w in want]
    return out


# ------------------------------------------------------------------------------------------- (a) the reference's own answers
def test_conflicting_moves():
    """crates/loro/tests/mov.rs:13-62, the script of test_emu_movable.known_answer_docs"""
    d1 = wire.Replica(1)
    for i, v in enumerate((1, 2, 3)):
        d1.mlist_insert("list", i, [v])
    d2 = wire.Replica(2)
    take(d2, d1)
    assert model_of(d1).value() == {"list": [1, 2, 3]}
    d1.mlist_move("list", 0, 2); d2.mlist_move("list", 0, 1)
    d1.commit(); d2.commit()
    m = model_of(d1, d2)
    assert m.json() == b'{"list":[2,1,3]}'
    assert len(m.visible_ids(wire.root_cid("list", ML))) == 4          # the losing move's item stays, pointed at by nothing
    assert m.movable_outcomes()["move_tie_on_lamport"] == 1 and m.movable_outcomes()["loser_item_alive"] == 1


def test_handler_ops_of_one_peer():
    """state/movable_list_state.rs:1940-1958 and :1960-2031, every intermediate value as a checkout"""
    d = wire.Replica(7)
    steps = []
    def then(want):
        steps.append((d.next_counter - 1, want))
    for i in range(3):
        d.mlist_insert("list", i, [i])
    then([0, 1, 2])
    d.mlist_move("list", 0, 1); then([1, 0, 2])
    d.mlist_move("list", 2, 0); then([2, 1, 0])
    d.mlist_delete("list", 0, 2); then([0])
    d.mlist_insert("list", 0, [9]); then([9, 0])
    d.mlist_delete("list", 0, 2); then([])
    d.commit()
    m = model_of(d)
    for ctr, want in steps:
        assert m.value([(7, ctr)]) == {"list": want}, ctr
    assert m.json() == b'{"list":[]}'
    d = wire.Replica(8)
    steps = []
    d.mlist_insert("list", 0, [1]); d.mlist_insert("list", 1, [0]); d.mlist_move("list", 0, 1); then([0, 1])
    d.mlist_move("list", 1, 0); then([1, 0])
    d.mlist_move("list", 0, 1); d.mlist_insert("list", 2, [3]); d.mlist_set("list", 2, 2); then([0, 1, 2])
    d.commit()
    m = model_of(d)
    for ctr, want in steps:
        assert m.value([(8, ctr)]) == {"list": want}, ctr
    assert m.json() == b'{"list":[0,1,2]}'


def test_runtime_fixture_script_and_emptied_list():
    """what wrote the runtime fixture (loro-js/scripts/rewrite-rust-fixture.mjs:73-77: push x, push y, move(0, 1), set(0, "z")) ->
    runtime.expected.json's ["z","x"]; a MovableList that was emptied is still shown, an emptied List is not"""
    r = wire.Replica(3)
    r.mlist_insert("movable", 0, ["x"]); r.mlist_insert("movable", 1, ["y"]); r.mlist_move("movable", 0, 1); r.mlist_set("movable", 0, "z")
    r.commit()
    assert model_of(r).json() == b'{"movable":["z","x"]}'
    e = wire.Replica(9)
    e.mlist_insert("gone", 0, ["a", "b"]); e.mlist_delete("gone", 0, 2); e.list_insert("l", 0, [1]); e.list_delete("l", 0, 1)
    e.commit()
    assert model_of(e).json() == b'{"gone":[]}'


def test_existence_and_nesting_known_answers():
    """test_emu_movable.existence_docs and nesting_docs, from the same scripts"""
    r = wire.Replica(31)
    r.map_set("m", "k", 1); r.commit(); v1 = list(r.frontiers)
    r.mlist_insert("ml", 0, ["a", "b"]); r.commit(); v2 = list(r.frontiers)
    r.mlist_move("ml", 0, 1); r.mlist_set("ml", 0, "B"); r.commit(); v3 = list(r.frontiers)
    r.mlist_delete("ml", 0, 2); r.commit()
    m = model_of(r)
    assert [m.json(v) for v in (None, v1, v2, v3, [])] == [b'{"m":{"k":1},"ml":[]}', b'{"m":{"k":1},"ml":[]}', b'{"m":{"k":1},"ml":["a","b"]}',
                                                           b'{"m":{"k":1},"ml":["B","a"]}', b'{"m":{},"ml":[]}']
    r = wire.Replica(5)
    r.map_set_container("m", "never", ML)
    inl = r.list_insert_container("l", 0, ML)
    r.mlist_insert(inl, 0, [1, 2, 3]); r.mlist_move(inl, 2, 0)
    inner = r.mlist_insert_container(inl, 1, ML)
    r.mlist_insert(inner, 0, ["x", "y"]); r.mlist_move(inner, 0, 1); r.mlist_set(inner, 0, "Y")
    setc = r.mlist_set_container(inl, 3, wire.KIND_TEXT)
    r.text_insert(setc, 0, "hi")
    r.commit()
    assert model_of(r).json() == b'{"l":[[3,["Y","x"],1,"hi"]],"m":{"never":[]}}'


def test_sliced_script():
    """test_emu_movable.sliced_docs' history, whole"""
    r = wire.Replica(7)
    r.mlist_insert("ml", 0, ["a", "b", "c"]); r.mlist_move("ml", 0, 2); r.mlist_set("ml", 0, "B")
    r.mlist_insert("ml", 1, ["d"]); r.mlist_delete("ml", 0, 1); r.mlist_move("ml", 2, 0); r.mlist_set("ml", 1, "D")
    r.commit()
    assert model_of(r).json() == b'{"ml":["a","D","c"]}'


# ------------------------------------------------------------------------------------------- (b) the model against the oracle
def against_oracle(docs, all_versions):
    at = [(d, None, None) for d in docs] + [(d, fr, upd) for d in docs for fr, upd in d.snaps] + [(d, fr, None) for d in docs for fr in d.versions]
    if not all_versions:
        at = [(d, fr, upd) for d, fr, upd in at if fr is None or upd is not None or fr in d.versions[:2]]
    got = _oracle.merge_batch([d.blobs for d, _, _ in at], threads=8, frontiers=[None if fr is None else wire.encode_frontiers(fr) for _, fr, _ in at])
    for (d, fr, upd), g in zip(at, got):
        assert g == d.model.result(fr), (d.label, fr, g, d.model.result(fr))
        ids_of = d.blobs if fr is None else (upd and [upd])          # (updates that hold exactly this version: the oracle's ids of it)
        if ids_of is not None:
            for cid in d.model.sequences():
                assert _oracle.visible_ids(ids_of, cid, cid.kind) == d.model.visible_ids(cid, fr), (d.label, fr, cid)
    return len(at)


@pytest.mark.parametrize("name", ["movable", "movable nested", "movable 5 peers"])
def test_model_against_oracle(corpora, name):
    docs = corpora[name]
    assert against_oracle(docs, True) >= 4 * len(docs)
    against_oracle(_merge_docs.overlapping_docs(docs[:10]), False)


def test_hand_built_against_oracle(hand_built):
    for docs in hand_built.values():
        against_oracle(docs, True)


# ------------------------------------------------------------------------------------------- (c) the model against the kernel-logic harness
CONFIGS = [{"LM_SPAN": "1"}, {"LM_SPAN": "0"}, {"LM_DECODE": "0"}, {"LM_DIR_OPT_MAX": "4"}]


@pytest.mark.parametrize("env", CONFIGS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_model_against_harness(corpora, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    docs = [d for ds in corpora.values() for d in ds]
    docs += _merge_docs.overlapping_docs([ds[i] for ds in corpora.values() for i in range(0, 10)])
    labels, blobs, fronts, want = entries(docs, "LM_SPAN" in env, n_versions=2)
    compare(_emu.merge_batch(blobs, fronts), labels, blobs, fronts, want, env)      # (these lists are short: no retry is forced here)


@pytest.mark.parametrize("env", CONFIGS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_hand_built_against_harness(hand_built, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    retried = 0
    for name, docs in hand_built.items():
        labels, blobs, fronts, want = entries(docs, True, n_versions=99)
        with Context(_emu.binding()) as c:
            compare(c.merge_batch(blobs, fronts), labels, blobs, fronts, want, (name, env))
            retried += c.sizing()[3]
    assert "LM_DIR_OPT_MAX" not in env or retried >= 1
