"""MovableList deltas between two versions (lm_delta_movable): the plain reference, from the merge model alone (_merge_ref.py), and the
cases shared by the kernel-logic (CPU) and the GPU tests.

The definition (include/loro_merge.h), restated literally over `model.seqs`, `model.elems`, `_visible` and `_greatest`:
  * an ITEM is an entry of `model.seqs[cid]` (an insert atom or a move), in sequence order; el(i) = `item.what[1]`;
  * pos_X(e) = `_greatest` of e's insert and its moves in X, val_X(e) = `_greatest` of e's insert and its sets in X;
  * item i shows at X iff id(i) in X, i is pos_X(el(i)), and no DELETE atom in X targets i.  The model also books a move as a deleter of
    the item it took the element from; `shows` leaves those out, as the definition does, and asserts that the walk of `Model._value`
    (which counts them, `_visible`) shows exactly the same items: the winner of X is never an item a move in X deleted;
  * K / R / I / D, from_move and the canonical form as in the header.
Values go through `_values.to_json` (a child container: the parrot string of the writing op's ContainerID, `_delta_map.shallow_json`) and
`_delta_map.values_equal`.  Every result is compared byte for byte, then — independent of the form — the ops are applied to the shallow
value at A and must give the shallow value at V; a from_move insert must carry a value the same delta deleted."""
import json
import random

import _cursor, _delta_map, _fuzz, _merge_docs, _merge_ref
from _delta_map import OK, DECODE_ERROR, UNSUPPORTED, FRONTIERS_NOT_FOUND, cid_str, shallow_json, values_equal, vv_ids
from _merge_ref import _greatest, _visible
from _richtext_ref import changes_of
from _values import to_json
from loro_amd import wire

ML = _merge_docs.ML
OUTCOMES = ("kept", "from_move", "moved_and_set", "replaced", "inserted", "gone", "set_equal", "undecided")
# asserted per corpus, from the model alone, before anything is compared: a corpus must not pass by being boring
AT_LEAST = {"kept": 2000, "from_move": 500, "moved_and_set": 200, "replaced": 400, "inserted": 10000, "gone": 900, "set_equal": 4}
QUERIES = {"movable": 520, "movable nested": 299, "movable 5 peers": 532}


# ---- the definition, restated
def _move_ids(model, cid):
    return {m[2] for el in model.elems[cid].values() for m in el.moves}


def pos_at(el, X):
    """the item id of the element's position winner at X, None when X does not hold its insert"""
    if el.insert[2] not in X:
        return None
    return _greatest([el.insert[:3]] + [m for m in el.moves if m[2] in X])[2]


def val_at(el, X):
    """(lamport, peer, op id, value) of the element's value winner at X"""
    return _greatest([el.insert] + [s for s in el.sets if s[2] in X])


def shows(model, cid, X):
    """[bool] per item of `model.seqs[cid]`: the definition's three conditions"""
    moves = _move_ids(model, cid)
    out, walk = [], []
    for it in model.seqs[cid]:
        el = model.elems[cid][it.what[1]]
        deleted = any(dl in X and dl not in moves for dl in it.deleters)
        out.append(it.id in X and pos_at(el, X) == it.id and not deleted)
        walk.append(_visible(it, X) and _greatest([el.insert[:3]] + [m for m in el.moves if m[2] in X])[2] == it.id)    # Model._value's walk
    assert out == walk, ("a winner that a move in the version deleted", cid)
    return out


def shallow_list(model, cid, X):
    """the parsed shallow value of the list at X"""
    return [json.loads(shallow_json(val_at(model.elems[cid][it.what[1]], X))) for it, s in zip(model.seqs[cid], shows(model, cid, X)) if s]


def container_delta(model, cid, A, V, counts):
    """(list of op JSON texts, undecided) of one MovableList between the id sets A and V"""
    sa, sv = shows(model, cid, A), shows(model, cid, V)
    elems = model.elems[cid]
    shown_a = {it.what[1] for it, s in zip(model.seqs[cid], sa) if s}          # elements that show at A, at whichever item
    shown_v = {it.what[1] for it, s in zip(model.seqs[cid], sv) if s}
    ops, undecided = [], False
    retain, ins, dele = 0, [], 0          # ins: [(flag, [json text])]

    def close_gap():
        nonlocal dele
        for flag, vals in ins:
            ops.append('{"insert":[%s]%s}' % (",".join(vals), ',"from_move":true' if flag else ""))
        del ins[:]
        if dele:
            ops.append('{"delete":%d}' % dele)
            dele = 0

    for it, a, v in zip(model.seqs[cid], sa, sv):
        if not a and not v:
            continue
        name = it.what[1]
        el = elems[name]
        wa, wv = val_at(el, A), val_at(el, V)
        same = None
        if name in shown_a and v:
            if wa[2] == wv[2]:
                same = True
            else:
                same = values_equal(wa[3], wv[3])
                if same is None:
                    undecided, same = True, False
                    counts["undecided"] += 1
                counts["set_equal"] += bool(same)
        if a and v and same:
            counts["kept"] += 1
            if ins or dele:
                close_gap()
            retain += 1
            continue
        if retain and not (ins or dele):
            ops.append('{"retain":%d}' % retain)
        retain = 0
        if a:
            dele += 1
            if not v:
                counts["gone"] += name not in shown_v
        if v:
            flag = bool(not a and name in shown_a and same)
            if a:
                counts["replaced"] += 1
            elif flag:
                counts["from_move"] += 1
            elif name in shown_a:
                counts["moved_and_set"] += 1
            else:
                counts["inserted"] += 1
            if not ins or ins[-1][0] != flag:
                ins.append((flag, []))
            ins[-1][1].append(shallow_json(wv))
    close_gap()
    return ops, undecided


def expected(model, A, V):
    """(bytes, other_changed, outcome counts) lm_delta_movable must give between the id sets A and V"""
    members, counts, undecided = {}, dict.fromkeys(OUTCOMES, 0), False
    for cid in model.elems:
        ops, und = container_delta(model, cid, A, V, counts)
        undecided |= und
        if ops:
            members[to_json(cid_str(cid))] = "[" + ",".join(ops) + "]"
    other = 0
    for ch in model.changes:
        for op in ch.ops:
            if op.cid.kind in (wire.KIND_TREE, wire.KIND_COUNTER):
                other |= any((ch.peer, op.counter + i) in V and (ch.peer, op.counter + i) not in A for i in range(op.atom_len))
    body = ",".join("%s:%s" % (k, members[k]) for k in sorted(members, key=lambda k: k.encode("utf-8")))
    return ("{" + body + "}").encode("utf-8"), (1 if other else 0) | (2 if undecided else 0), counts


def apply_ops(value, ops, what=""):
    """the ops applied to a list; from_move plays no part here, except that such an insert must carry a value the delta deleted"""
    out, at, deleted, moved = list(value), 0, [], []
    for op in ops:
        if "retain" in op:
            at += op["retain"]
            assert at <= len(out), what
        elif "insert" in op:
            assert op["insert"] and set(op) <= {"insert", "from_move"} and op.get("from_move", True) is True, (what, op)
            out[at:at] = op["insert"]
            at += len(op["insert"])
            if op.get("from_move"):
                moved += op["insert"]
        else:
            assert set(op) == {"delete"} and op["delete"] > 0 and at + op["delete"] <= len(out), (what, op)
            deleted += out[at:at + op["delete"]]
            del out[at:at + op["delete"]]
    for v in moved:
        assert any(type(v) is type(x) and v == x for x in deleted), (what, "a from_move insert whose value the delta did not delete", v)
    assert not ops or "retain" not in ops[-1], (what, "a trailing retain")
    return out


def check_one(got, model, A, V, what=""):
    """one result (status, other_changed, bytes) against the reference: the bytes, then the applier"""
    want, oc, _ = expected(model, A, V)
    assert got[0] == OK, (what, got)
    assert got[2] == want, (what, got[2], want)
    assert got[1] == oc, (what, got[1], oc)
    delta = json.loads(got[2])
    names = {cid_str(cid): cid for cid in model.elems}
    assert set(delta) <= set(names), what
    for name, cid in names.items():
        assert apply_ops(shallow_list(model, cid, A), delta.get(name, []), (what, name)) == shallow_list(model, cid, V), (what, name)


# ---- corpora: A = the empty version plus every recorded version, V = latest
def corpus_queries(docs):
    return [(i, fr) for i, d in enumerate(docs) for fr in [[]] + d.versions]


def check_conditions(name, docs, queries):
    tot = dict.fromkeys(OUTCOMES, 0)
    for i, fr in queries:
        m = docs[i].model
        for k, v in expected(m, m.version(fr), m.all_ids)[2].items():
            tot[k] += v
    assert len(queries) == QUERIES[name], (name, len(queries))
    for k, least in AT_LEAST.items():
        assert tot[k] >= least, (name, k, tot)
    return tot


def run_docs(ctx, docs, queries, what=""):
    """[(document index, frontiers of A or None for the empty version)] on `docs` rendered at the latest version"""
    res = ctx.merge_batch([d.blobs for d in docs])
    assert res == [d.model.result() for d in docs], what
    got = ctx.delta_movable([(i, docs[i].model.vv(fr)) for i, fr in queries])
    for (i, fr), g in zip(queries, got):
        m = docs[i].model
        check_one(g, m, m.version(fr), m.all_ids, (what, docs[i].label, fr))
    assert ctx.fetch() == res, what
    return len(queries)


def inside_and_ends(doc):
    """the empty version, the end of every change and every counter inside the changes of a (small) document — each a single id,
    closed over its dependencies by the model — plus the versions the document records"""
    out = [[]] + [list(fr) for fr in doc.versions]
    for c in doc.model.changes:
        for k in range(c.counter, c.ctr_end):
            if [(c.peer, k)] not in out:
                out.append([(c.peer, k)])
    return out


# ---- hand cases with exact bytes
def _root(body):
    return b'{"cid:root-ml:MovableList":' + body + b"}"


def _abc(peer):
    r = wire.Replica(peer)
    r.mlist_insert("ml", 0, ["a", "b", "c"]); r.commit()
    return r, dict(r.vv)


def hand_cases():
    """(name, replicas or (blobs, model), [(A as {peer: counter} or None, expected bytes, other_changed)])"""
    out = []
    r, a = _abc(5); r.mlist_move("ml", 0, 2); r.commit()
    out.append(("move index 0 to the end", [r], [(a, _root(b'[{"delete":1},{"retain":2},{"insert":["a"],"from_move":true}]'), 0),
                                                 (None, _root(b'[{"insert":["b","c","a"]}]'), 0), (dict(r.vv), b"{}", 0)]))
    r, a = _abc(6); r.mlist_move("ml", 0, 2); r.mlist_insert("ml", 3, ["x"]); r.commit()
    out.append(("… then insert x at the end", [r], [(a, _root(b'[{"delete":1},{"retain":2},{"insert":["a"],"from_move":true},{"insert":["x"]}]'), 0)]))
    r, a = _abc(7); r.mlist_move("ml", 0, 2); r.mlist_set("ml", 2, "A"); r.commit()
    out.append(("move index 0 to the end and set it", [r], [(a, _root(b'[{"delete":1},{"retain":2},{"insert":["A"]}]'), 0)]))
    r, a = _abc(8); r.mlist_set("ml", 1, "B"); r.commit()
    out.append(("set index 1", [r], [(a, _root(b'[{"retain":1},{"insert":["B"]},{"delete":1}]'), 0)]))
    r, a = _abc(9); r.mlist_set("ml", 1, "b"); r.commit()
    out.append(("set index 1 to an equal value", [r], [(a, b"{}", 0)]))
    r, a = _abc(10); r.mlist_delete("ml", 1, 1); r.mlist_insert("ml", 0, ["x"]); r.commit()
    out.append(("delete index 1, insert x at 0", [r], [(a, _root(b'[{"insert":["x"]},{"retain":1},{"delete":1}]'), 0)]))
    r, a = _abc(11); r.mlist_move("ml", 0, 2); r.mlist_set("ml", 2, "a"); r.commit()
    out.append(("moved and set to an equal value: still from_move", [r], [(a, _root(b'[{"delete":1},{"retain":2},{"insert":["a"],"from_move":true}]'), 0)]))
    r = wire.Replica(12); r.mlist_insert("ml", 0, ["a", "b", "c", "d", "e"]); r.commit(); a = dict(r.vv)
    r.mlist_delete("ml", 1, 3); r.commit()
    out.append(("a delete run cut by A after its first atom", [r], [(a, _root(b'[{"retain":1},{"delete":3}]'), 0), ({12: 6}, _root(b'[{"retain":1},{"delete":2}]'), 0),
                                                                    ({12: 7}, _root(b'[{"retain":1},{"delete":1}]'), 0)]))
    r = wire.Replica(13); r.mlist_insert("ml", 0, [[1, 2], {"k": 1}, "s"]); r.commit(); a = dict(r.vv)
    r.mlist_set("ml", 0, [1, 2]); r.mlist_set("ml", 1, {"k": 1}); r.commit()
    out.append(("nested List over nested List, nested Map over nested Map: not decided, replaced", [r],
                [(a, _root(b'[{"insert":[[1,2],{"k":1}]},{"delete":2}]'), 2)]))
    r = wire.Replica(14); r.map_set("m", "k", 1); r.text_insert("t", 0, "x"); r.list_insert("l", 0, [1]); r.mlist_insert("ml", 0, ["a"]); r.commit(); a = dict(r.vv)
    r.map_set("m", "k", 2); r.text_insert("t", 0, "y"); r.list_insert("l", 0, [2]); r.commit(); a2 = dict(r.vv)
    r.mlist_insert("ml", 1, [1.5, None, True, b"\x01"]); r.commit()
    out.append(("Text, List and Map ops set nothing", [r], [(a, _root(b'[{"retain":1},{"insert":[1.5,null,true,[1]]}]'), 0), (a2, _root(b'[{"retain":1},{"insert":[1.5,null,true,[1]]}]'), 0)]))
    r, a = _abc(15)
    ct = r.mlist_set_container("ml", 1, wire.KIND_TEXT); r.text_insert(ct, 0, "kid")
    ci = r.mlist_insert_container("ml", 0, wire.KIND_MAP); r.commit()
    want = ('[{"insert":["%s:cid:%d@15:Map"]},{"retain":1},{"insert":["%s:cid:%d@15:Text"]},{"delete":1}]' % (_delta_map.PARROT, ci.counter, _delta_map.PARROT, ct.counter)).encode("utf-8")
    out.append(("a child made by a set and a child made by an insert", [r], [(a, _root(want), 0)]))
    # a nested MovableList under its own ContainerID
    r = wire.Replica(16); inner = r.mlist_insert_container("ml", 0, wire.KIND_MOVABLE); r.mlist_insert(inner, 0, [1, 2]); r.commit(); a = dict(r.vv)
    r.mlist_move(inner, 0, 1); r.commit()
    want = ('{"cid:%d@16:MovableList":[{"delete":1},{"retain":1},{"insert":[1],"from_move":true}]}' % inner.counter).encode()
    out.append(("a child MovableList is listed under its own id", [r], [(a, want, 0)]))
    # a pending change delivered in V's blobs: c depends on b, whose blob is missing
    a_, b_, c_ = wire.Replica(30), wire.Replica(20), wire.Replica(10)
    a_.mlist_insert("ml", 0, ["a", "b"]); a_.commit()
    b_.merge_from(a_); b_.set_visible(ML, ML.kind, _merge_ref.view(b_, ML)); b_.mlist_move("ml", 0, 1); b_.commit()
    c_.merge_from(b_); c_.set_visible(ML, ML.kind, _merge_ref.view(c_, ML)); c_.mlist_set("ml", 0, "late"); c_.mlist_move("ml", 1, 0); c_.commit()
    blobs = [a_.export(), c_.export(dict(b_.vv))]
    model = _merge_ref.Model(changes_of([a_, b_, c_]), delivered=a_.changes[30] + c_.changes[10])
    assert model.pending == 2
    out.append(("a pending change delivered in V's blobs does not compete", (blobs, model), [(None, _root(b'[{"insert":["a","b"]}]'), 0)]))
    r, a = _abc(21); first = r.export()
    r.mlist_move("ml", 2, 0); r.mlist_set("ml", 1, "A"); r.commit()
    out.append(("a duplicated blob", ([first, r.export(), first, r.export()], _merge_ref.Model(changes_of([r]))),
                [(a, _root(b'[{"insert":["c"],"from_move":true},{"insert":["A"]},{"delete":1},{"retain":1},{"delete":1}]'), 0)]))
    return out


def _case_doc(case):
    src = case[1]
    if isinstance(src, tuple):
        return src
    return _fuzz.blobs_of(src), _merge_ref.Model(changes_of(src))


def run_hand_cases(ctx):
    cases = hand_cases()
    built = [_case_doc(c) for c in cases]
    docs = [b for b, _ in built]
    docs.append([docs[0][0][:-2] + b"\x00\x01"])            # a document whose import fails, next to healthy ones
    res = ctx.merge_batch(docs)
    assert [r for r in res[:-1]] == [m.result() for _, m in built] and res[-1][0] != 0
    qs, want, info = [], [], []
    for d, (name, _, queries) in enumerate(cases):
        for a, exp, oc in queries:
            qs.append((d, None if a is None else wire.encode_vv(a)))
            want.append((OK, oc, exp))
            info.append((name, d, a))
    got = ctx.delta_movable(qs)
    for i, g, w in zip(info, got, want):
        assert g == w, (i[0], i[2], g, w)
    # … and the hand-written bytes agree with the derived reference, and apply
    for (name, d, a), w, g in zip(info, want, got):
        m = built[d][1]
        e = expected(m, vv_ids(a or {}), m.all_ids)
        assert (e[0], e[1]) == (w[2], w[1]), (name, e[:2], w)
        check_one(g, m, vv_ids(a or {}), m.all_ids, name)
    # statuses
    f = len(docs) - 1
    vv0 = res[0][2]
    peer, ctr = next(iter(_cursor.decode_vv(vv0).items()))
    enc = wire.encode_vv
    got = ctx.delta_movable([(f, None), (0, enc({peer: ctr + 1})), (0, enc({peer: ctr, 424242: 1})), (0, enc({peer: ctr, 424242: 0})), (0, vv0[:-1]), (0, vv0 + b"\x00")])
    assert got[0][0] == res[-1][0] and got[0][2] == b""
    assert [g[0] for g in got[1:]] == [FRONTIERS_NOT_FOUND, FRONTIERS_NOT_FOUND, OK, DECODE_ERROR, DECODE_ERROR], got
    assert got[3][2] == b"{}"
    assert ctx.fetch() == res
    try:
        ctx.delta_movable([(len(docs), None)])
    except RuntimeError:
        pass
    else:
        raise AssertionError("a call that cannot be answered must return -1")
    # lm_delta and lm_delta_map report a MovableList's ops as before (other_changed), whichever call ran in between
    every = [(d, None) for d in range(len(cases))]
    before, before_map = ctx.delta(every), ctx.delta_map(every)
    assert all(g[1] == 1 and b"MovableList" not in g[2] for g in before) and all(g[1] & 1 and b"MovableList" not in g[2] for g in before_map)
    assert ctx.delta_movable(qs) == want and ctx.delta(every) == before and ctx.delta_map(every) == before_map and ctx.delta_movable(qs) == want
    assert ctx.fetch() == res


# ---- the hand-built documents of _merge_docs, queried at A = empty, at every change end and inside changes
def hand_built():
    out = {"ties": _merge_docs.lamport_tie_docs(), "delete": _merge_docs.move_against_delete_docs()[0], "split": [_merge_docs.split_maxima_docs()[0]],
           "children": _merge_docs.children_docs()[0]}
    return out


def run_hand_built(ctx, groups, what=""):
    n = 0
    for name, docs in groups.items():
        n += run_docs(ctx, docs, [(i, fr) for i, d in enumerate(docs) for fr in inside_and_ends(d)], (what, name))
    return n


def run_row_passes(ctx, docs, what=""):
    """63 / 64 / 65 / 129 move rows: runs and gaps across chunk and leaf edges; A = empty, the recorded versions (inside the long change, on
    both sides of a pass boundary) and the end of the base"""
    def base_end(d):
        c = d.reps[0].changes[d.reps[0].peer][0]
        return [(c.peer, c.ctr_end - 1)]
    return run_docs(ctx, docs, [(i, fr) for i, d in enumerate(docs) for fr in [[]] + d.versions + [base_end(d)]], what)


def run_table_load(ctx, doc, what=""):
    """1,500 elements each moved and set: table load and a list of many leaves, from the end of the base, the empty version and the
    recorded versions"""
    return run_docs(ctx, [doc], [(0, fr) for fr in [[(doc.reps[0].peer, 1499)], []] + doc.versions], what)


def run_overflow(ctx):
    """every other of 600 small values deleted and a few moved: the delta ({"retain":1},{"delete":1},… ) is several times the document's
    JSON and larger than the optimistic slab — the second launch, at exact sizes"""
    r = wire.Replica(51)
    r.mlist_insert("ml", 0, list(range(600))); r.commit(); a = dict(r.vv)
    for i in range(299, -1, -1):
        r.mlist_delete("ml", 2 * i + 1, 1)
    for i in range(0, 40, 4):
        r.mlist_move("ml", i, 299 - i)
    r.commit()
    m = _merge_ref.Model(changes_of([r]))
    want = expected(m, vv_ids(a), m.all_ids)[0]
    ctx.set_profiling(1)
    res = ctx.merge_batch([[r.export()]])
    assert res == [m.result()] and len(want) > 2 * len(res[0][1]) + 2048
    check_one(ctx.delta_movable([(0, wire.encode_vv(a))])[0], m, vv_ids(a), m.all_ids, "slab overflow")
    assert ctx.b.delta_bytes(ctx.h) == ((len(want) + 15) & ~15) + 2 * 16                  # the bytes written + a result row per launch
    assert [n for n, _ in ctx.kernel_times()].count("k_mldelta") == 2                      # the second launch, at exact sizes
    ctx.set_profiling(0)
    assert ctx.fetch() == res


def run_without_a_movable_list(ctx, monkeypatch):
    """documents that hold no MovableList answer {} with other_changed 0: a Text / List document through the kernels, an LWW Map document
    decoded without op rows on the host; next to them a document that has one"""
    import _merge_docs_map
    for k, v in _merge_docs_map.FORCE.items():
        monkeypatch.setenv(k, v)
    t = wire.Replica(77); t.text_insert("t", 0, "no list here"); t.list_insert("l", 0, [1, 2]); t.commit()
    m = wire.Replica(78)
    for i in range(40):
        m.map_set("m", "k%d" % (i % 7), i)
    m.commit()
    r, a = _abc(79); r.mlist_move("ml", 0, 2); r.commit()
    res = ctx.merge_batch([[t.export()], [m.export()], [r.export()]])
    assert [x[0] for x in res] == [0, 0, 0]
    fused = ctx.b.fused_documents(ctx.h)
    got = ctx.delta_movable([(0, None), (1, None), (1, wire.encode_vv({78: 5})), (2, wire.encode_vv(a)), (0, wire.encode_vv(dict(t.vv)))])
    assert got[:3] == [(OK, 0, b"{}")] * 3 and got[4] == (OK, 0, b"{}"), got
    assert got[3] == (OK, 0, _root(b'[{"delete":1},{"retain":2},{"insert":["a"],"from_move":true}]'))
    assert ctx.b.fused_documents(ctx.h) == fused and ctx.fetch() == res        # (the Map document was not run again for this call)
    return fused


# ---- a document with Tree / Counter ops: other_changed bit 0.  loro_amd.wire writes no such op; tests/golden/reference_fixtures.json
# holds blobs the reference shipped that do (lm_fetch reports them LM_UNSUPPORTED together with their JSON; the delta calls answer them)
def _fixture(name):
    import os
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures.json")))["blobs"]
    return bytes.fromhex(fx[name])


def run_tree_and_counter_ops(ctx):
    """runtime-updates.ts.blob: ONE change of peer 42, written by loro-js/scripts/rewrite-rust-fixture.mjs:57-83 — Map, List and Text ops
    (one of them a mergeable Counter's increment), then movable.push("x") at counter 20, push("y") 21, move(0, 1) 22, set(0, "z") 23, then
    a Counter increment and three Tree ops, 24-27.  The expected bytes are worked out from that script by the definition: the items
    stand as [x's insert][y][x's move]; bit 0 is set for every A short of V (the last four ops are Counter / Tree ops) and clear at V.
    updates.blob (three peers, Rust-written, its script is not held here): from the empty version the nested list's whole content —
    the values of "child_mlist" in the document's JSON, its child Text as the parrot string — with bit 0; and along the cuts of peer 1
    (the other peers at their ends) bit 0, "a Tree / Counter op lies in V \\ A", can only go from set to clear, is set at 0, and is
    clear for the last cuts short of V, which the kernels answer (A != V)."""
    rt, up = _fixture("runtime-updates.ts.blob"), _fixture("updates.blob")
    res = ctx.merge_batch([[rt], [up], [_fixture("runtime-snapshot.ts.blob")]])
    assert [r[0] for r in res] == [UNSUPPORTED] * 3 and all(len(r[1]) > 2 for r in res)           # the document's own status, with its JSON
    assert _cursor.decode_vv(res[0][2]) == {42: 28} and _cursor.decode_vv(res[1][2]) == {1: 46, 2: 11, 3: 7}
    key = b'{"cid:root-movable:MovableList":'
    want = {0: b'[{"insert":["z","x"]}]', 20: b'[{"insert":["z","x"]}]',
            21: b'[{"insert":["z"]},{"insert":["x"],"from_move":true},{"delete":1}]',        # A = [x]:    x's insert D, y I, x's move I from_move
            22: b'[{"insert":["z"]},{"insert":["x"],"from_move":true},{"delete":2}]',        # A = [x, y]: x's insert D, y R, x's move I from_move
            23: b'[{"insert":["z"]},{"delete":1}]',                                          # A = [y, x]: y R, x's move K (trailing retain dropped)
            24: None, 25: None, 27: None}
    for doc in (0, 2):                                   # the updates and the snapshot form of the same document
        ks = sorted(want)
        got = ctx.delta_movable([(doc, wire.encode_vv({42: k}) if k else None) for k in ks] + [(doc, res[doc][2])])
        for k, g in zip(ks, got):
            assert g == (OK, 1, b"{}" if want[k] is None else key + want[k] + b"}"), (doc, k, g)
        assert got[-1] == (OK, 0, b"{}"), got[-1]
    got = ctx.delta_movable([(1, None)] + [(1, wire.encode_vv({1: k, 2: 11, 3: 7})) for k in range(46)] + [(1, res[1][2])])
    assert got[0] == (OK, 1, ('{"cid:25@1:MovableList":[{"insert":["%s:cid:3@3:Text",166163940,1551498871,20,10]}]}' % _delta_map.PARROT).encode("utf-8")), got[0]
    assert b'"child_mlist":["",166163940,1551498871,20,10]' in res[1][1]
    bits = [g[1] & 1 for g in got[1:47]]
    assert all(g[0] == OK for g in got) and bits[0] == 1 and bits == sorted(bits, reverse=True) and bits[-1] == 0, bits
    assert got[-1] == (OK, 0, b"{}")
    assert ctx.fetch() == res


def run_bytes_moved(ctx):
    """what crosses to the host is proportional to the change: one move in a 1,000-item list copies back under 256 bytes"""
    r = wire.Replica(52)
    r.mlist_insert("ml", 0, list(range(1000))); r.commit(); a = dict(r.vv)
    r.mlist_move("ml", 10, 500); r.commit()
    res = ctx.merge_batch([[r.export()]])
    assert len(res[0][1]) > 3000
    want = _root(b'[{"retain":10},{"delete":1},{"retain":490},{"insert":[10],"from_move":true}]')
    assert ctx.delta_movable([(0, wire.encode_vv(a))]) == [(OK, 0, want)]
    assert ctx.b.delta_bytes(ctx.h) == ((len(want) + 15) & ~15) + 16 < 256
    assert ctx.fetch() == res


def steps(seed=5):
    """a two-writer MovableList history exported at three versions of the first writer: (export, frontiers, vv) each"""
    rng = random.Random(seed)
    r, o = wire.Replica(31), wire.Replica(32)
    r.mlist_insert("ml", 0, list("abcdefgh")); r.commit()
    o.merge_from(r); o.set_visible(ML, ML.kind, _merge_ref.view(o, ML))

    def write(w, n):
        for _ in range(n):
            ln, x = w.mlist_len("ml"), rng.random()
            if x < 0.35 and ln > 1:
                w.mlist_move("ml", rng.randrange(ln), rng.randrange(ln))
            elif x < 0.6 and ln:
                w.mlist_set("ml", rng.randrange(ln), rng.choice([1, "s", 2.5, None, "a"]))
            elif x < 0.75 and ln > 4:
                w.mlist_delete("ml", rng.randrange(ln - 1), rng.randint(1, 2))
            else:
                w.mlist_insert("ml", rng.randint(0, ln), [rng.randrange(100)])
            if rng.random() < 0.3:
                w.commit()
        w.commit()
    write(o, 25)
    out = []
    for s in range(3):
        write(r, 30)
        if s == 0:
            r.merge_from(o); r.set_visible(ML, ML.kind, _merge_ref.view(r, ML))
        out.append((r.export(), list(r.frontiers), dict(r.vv)))
    return out, _merge_ref.Model(changes_of([r]))


def run_checkout(ctx):
    ((_, _, v1), (_, f2, v2), (e3, _, v3)), model = steps()
    docs, fronts = [[e3], [e3]], [wire.encode_frontiers(f2), None]
    res = ctx.merge_batch(docs, fronts)
    assert res == [model.result(f2), model.result()]
    got = ctx.delta_movable([(0, wire.encode_vv(v1)), (1, wire.encode_vv(v1)), (0, wire.encode_vv(v2)), (0, wire.encode_vv(v3)), (1, wire.encode_vv(v2)), (0, None)])
    check_one(got[0], model, vv_ids(v1), model.version(f2), "checkout")
    check_one(got[1], model, vv_ids(v1), model.all_ids, "latest next to it")
    assert got[2][0] == OK and got[2][2] == b"{}"
    assert got[3][0] == FRONTIERS_NOT_FOUND                                  # A beyond the rendered version
    check_one(got[4], model, vv_ids(v2), model.all_ids, "latest from the checkout's version")
    check_one(got[5], model, frozenset(), model.version(f2), "checkout from the empty version")
    assert got[0][2] != b"{}" and got[4][2] != b"{}"
    assert ctx.fetch() == res


def resident_flow(ctx, n_docs=6):
    """stage + run, keep vv1 from fetch(); import_more + run, delta_movable(from vv1); a third step that brings a peer sorting in FRONT of
    the stored ones, queried from vv1 and from vv2"""
    reps, firsts, seconds, thirds, vv1m, vv2m = [], [], [], [], [], []
    for s in range(n_docs):
        rng = random.Random(900 + s)
        a, b, c = wire.Replica(7000 + s), wire.Replica(8000 + s), wire.Replica(100 + s)

        def write(w, n):
            for _ in range(n):
                ln, x = w.mlist_len("ml"), rng.random()
                if x < 0.35 and ln > 1:
                    w.mlist_move("ml", rng.randrange(ln), rng.randrange(ln))
                elif x < 0.6 and ln:
                    w.mlist_set("ml", rng.randrange(ln), rng.choice([rng.randrange(5), "v", 1.5, None, True]))
                elif x < 0.7 and ln > 3:
                    w.mlist_delete("ml", rng.randrange(ln), 1)
                else:
                    w.mlist_insert("ml", rng.randint(0, ln), [rng.randrange(100)])
                if rng.random() < 0.3:
                    w.commit()
            w.commit()

        def look(w):
            w.set_visible(ML, ML.kind, _merge_ref.view(w, ML))
        a.mlist_insert("ml", 0, list("abcdef")); a.commit()
        b.merge_from(a); look(b)
        write(a, 25); write(b, 15)
        firsts.append([a.export(), b.export(dict({a.peer: 6}))]); vv1m.append({**b.vv, **a.vv})
        c.merge_from(a); look(c)                               # the third writer has seen a's first step only
        have_c = dict(c.vv)
        a.merge_from(b); look(a); write(a, 20)
        seconds.append([a.export(vv1m[-1])]); vv2m.append(dict(a.vv))
        write(c, 15)
        thirds.append([c.export(have_c)])
        a.merge_from(c)
        reps.append(a)
    ctx.stage(firsts); ctx.run()
    r1 = ctx.fetch()
    vv1 = [r[2] for r in r1]
    assert vv1 == [wire.encode_vv(v) for v in vv1m]
    ctx.import_more(seconds); ctx.run()
    r2 = ctx.fetch()
    models = [_merge_ref.Model(changes_of([r])) for r in reps]
    assert [r[:3] for r in r2] == [m.result([(p, n - 1) for p, n in v.items()])[:3] for m, v in zip(models, vv2m)]
    got = ctx.delta_movable([(d, vv1[d]) for d in range(n_docs)])
    for d, g in enumerate(got):
        check_one(g, models[d], vv_ids(vv1m[d]), vv_ids(vv2m[d]), ("resident", d))
        assert g[2] != b"{}"
    assert ctx.fetch() == r2
    ctx.import_more(thirds); ctx.run()
    r3 = ctx.fetch()
    assert [r[:3] for r in r3] == [m.result()[:3] for m in models]
    got = ctx.delta_movable([(d, vv1[d]) for d in range(n_docs)] + [(d, r2[d][2]) for d in range(n_docs)])
    for d in range(n_docs):
        check_one(got[d], models[d], vv_ids(vv1m[d]), models[d].all_ids, ("resident, two imports back", d))
        check_one(got[n_docs + d], models[d], vv_ids(vv2m[d]), models[d].all_ids, ("resident, one import back", d))
        assert got[n_docs + d][2] != b"{}"
    assert ctx.fetch() == r3


def self_check_docs():
    """documents whose peers each END with a MovableList insert, move, set or delete (the skewed V lacks exactly that op)"""
    docs = []
    for k, last in enumerate(("insert", "move", "set", "delete")):
        a, b = wire.Replica(300 + k), wire.Replica(200 + k)
        a.mlist_insert("ml", 0, list("abcdef")); a.commit()
        b.merge_from(a); b.set_visible(ML, ML.kind, _merge_ref.view(b, ML))
        for r in (a, b):
            r.mlist_move("ml", 1, 4); r.mlist_set("ml", 2, "s%d" % r.peer); r.mlist_delete("ml", 0, 1); r.mlist_insert("ml", 2, ["i"])
            if last == "move":
                r.mlist_move("ml", 0, 3)
            elif last == "set":
                r.mlist_set("ml", 3, "last")
            elif last == "delete":
                r.mlist_delete("ml", 3, 1)
            r.commit()
        docs.append(_merge_docs.Doc("peers that end with a %s" % last, [a, b], [([(a.peer, 5)], None)], n_versions=2))
    return docs


def run_self_check(ctx, monkeypatch):
    """the self-check is the call's safety argument: with LM_DELTA_SKEW the device is handed a V one counter short for every peer — the
    status words, or the winners the run left, then disagree with the id sets, and every query must come back LM_UNSUPPORTED with no
    bytes; without the knob the same queries are answered"""
    docs = self_check_docs()
    res = ctx.merge_batch([d.blobs for d in docs])
    assert res == [d.model.result() for d in docs]
    queries = [(i, fr) for i, d in enumerate(docs) for fr in ([], [(d.reps[0].peer, 5)])]
    q = [(i, docs[i].model.vv(fr)) for i, fr in queries]
    good = ctx.delta_movable(q)
    for (i, fr), g in zip(queries, good):
        check_one(g, docs[i].model, docs[i].model.version(fr), docs[i].model.all_ids, docs[i].label)
        assert g[2] != b"{}"
    monkeypatch.setenv("LM_DELTA_SKEW", "1")
    assert ctx.delta_movable(q) == [(UNSUPPORTED, 0, b"")] * len(q)
    monkeypatch.delenv("LM_DELTA_SKEW")
    assert ctx.delta_movable(q) == good and ctx.fetch() == res


def run_snapshot(ctx):
    """a snapshot staged from its state section: the call stages it once more through its history (lm_delta's batch shapes)"""
    import _oracle
    snaps = []
    reps = _fuzz.movable_session(4100, snapshots=snaps, view=_merge_ref.view)
    d = _merge_docs.Doc("snapshot", reps, snaps)
    full = wire.Replica(reps[0].peer)
    for r in reps:
        full.merge_from(r)
    st, ents = _oracle.state_entries([full.export()])
    assert st == 0
    res = ctx.merge_batch([[full.export_snapshot(state=ents)]])
    assert ctx.b.state_documents(ctx.h) == 1 and res[0][:2] == d.model.result()[:2]
    frs = [[]] + d.versions
    got = ctx.delta_movable([(0, d.model.vv(fr)) for fr in frs])
    for fr, g in zip(frs, got):
        check_one(g, d.model, d.model.version(fr), d.model.all_ids, ("state-staged snapshot", fr))
    assert got[0][2] != b"{}"
    assert ctx.fetch() == res


# ---- rows racing for one table slot (GPU): 8 peers, each moving and setting the same `n_elems` elements 256 times
def race_doc(n_elems, n_peers=8, rounds=256):
    base = wire.Replica(5000)
    items = _merge_docs._raw_base(base, max(n_elems, 4) + 2)
    reps = [base]
    for p in range(n_peers):
        r = wire.Replica(6000 + 17 * p)
        r.merge_from(base)
        mine = list(items)
        for k in range(rounds):
            e = (base.peer, (k * 7 + p) % n_elems)
            _merge_docs._raw_move(r, ML, mine, e, (k * 5 + p * 3) % len(mine))
            _merge_docs._raw_set(r, ML, e, (k + p) % 3)            # (three values: many sets are equal to the one they replace)
            if k % 64 == 63:
                r.commit()
        r.commit()
        reps.append(r)
    return _merge_docs.Doc("%d peers race for %d elements" % (n_peers, n_elems), reps, [], n_versions=1)
