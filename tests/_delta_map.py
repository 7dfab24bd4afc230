"""Map deltas between two versions (lm_delta_map): the plain reference, from the merge model alone (_merge_ref.py), and the cases
shared by the kernel-logic (CPU) and the GPU tests.

  * the winner of a (Map, key) at a version = `Model.map_winner(cid, key, ids)`, ids = `Model.version(frontiers)` (or the id set of a
    version vector); A is sent as `Model.vv(frontiers)`;
  * the classification and the value equality are restated literally below (`classify`, `values_equal`);
  * values go through `_values.to_json`; a child container is the parrot string of its creating op's ContainerID;
  * every result is compared byte for byte, then — form-independent — `updated` / `deleted` applied to the shallow value of every Map
    at A must give its shallow value at V."""
import json
import math

import _cursor, _fuzz, _merge_docs_map, _merge_ref
from _merge_ref import _GONE
from _richtext_ref import changes_of
from _values import to_json
from loro_amd import wire

OK, DECODE_ERROR, UNSUPPORTED, FRONTIERS_NOT_FOUND = 0, 1, 4, 6
PARROT = "\U0001F99C"
KIND_NAMES = {wire.KIND_MAP: "Map", wire.KIND_LIST: "List", wire.KIND_TEXT: "Text", wire.KIND_TREE: "Tree", wire.KIND_MOVABLE: "MovableList", wire.KIND_COUNTER: "Counter"}
OUTCOMES = ("same_winner", "rewritten_equal", "updated", "deleted", "absent_then_set", "absent_then_delete", "delete_over_delete", "new_child", "undecided")
# asserted from the model alone before anything is compared: a corpus must not pass by being boring
AT_LEAST = {"rewritten_equal": 50, "delete_over_delete": 50, "same_winner": 500, "updated": 500, "deleted": 500, "absent_then_delete": 500, "new_child": 500}


def cid_str(cid):
    """ContainerID Display (loro-common/src/lib.rs)"""
    if cid.root:
        return "cid:root-%s:%s" % (cid.name, KIND_NAMES[cid.kind])
    return "cid:%d@%d:%s" % (cid.counter, cid.peer, KIND_NAMES[cid.kind])


# ---- the definition, restated
def _kind(v):
    if v is None:
        return "null"
    if isinstance(v, bool):
        return "bool"
    if isinstance(v, int):
        return "i64"
    if isinstance(v, float):
        return "f64"
    if isinstance(v, str):
        return "string"
    if isinstance(v, (bytes, bytearray)):
        return "binary"
    if isinstance(v, (list, tuple)):
        return "list"
    if isinstance(v, dict):
        return "map"
    assert isinstance(v, wire.ContainerValue), type(v)
    return "container"


def values_equal(a, b):
    """LoroValue equality (loro-common/src/value.rs:29-44) of the values of two DIFFERENT set ops: True / False, None = the device
    does not decide (two nested List values, two nested Map values)"""
    ka, kb = _kind(a), _kind(b)
    if ka != kb:
        return False                                # I64 3 and F64 3.0 differ
    if ka == "null":
        return True
    if ka in ("bool", "i64"):
        return a == b
    if ka == "f64":
        return a == b or (math.isnan(a) and math.isnan(b))      # 0.0 == -0.0
    if ka == "string":
        return a.encode("utf-8") == b.encode("utf-8")
    if ka == "binary":
        return bytes(a) == bytes(b)
    if ka == "container":
        return False                                # a ContainerID made from the creating op: two ops are never equal
    return None


def classify(wa, wv):
    """(outcome, reported as None | "updated" | "deleted" | "undecided") for the winners (lamport, peer, op id, value) at A and V"""
    if wv is None:
        return "absent", None
    if wa is not None and wa[2] == wv[2]:
        return "same_winner", None
    v_del = wv[3] is _GONE
    if wa is None:
        return ("absent_then_delete", "deleted") if v_del else ("absent_then_set", "updated")
    a_del = wa[3] is _GONE
    if a_del and v_del:
        return "delete_over_delete", None
    if v_del:
        return "deleted", "deleted"
    if a_del:
        return "updated", "updated"
    eq = values_equal(wa[3], wv[3])
    if eq is None:
        return "undecided", "undecided"
    return ("rewritten_equal", None) if eq else ("updated", "updated")


def shallow_json(w):
    """JSON text of a winning set's value; a child container is the parrot string of the creating op's ContainerID"""
    v = w[3]
    if isinstance(v, wire.ContainerValue):
        return to_json("%s:cid:%d@%d:%s" % (PARROT, w[2][1], w[2][0], KIND_NAMES[v.kind]))
    return to_json(v)


def vv_ids(vv):
    return frozenset((p, c) for p, n in vv.items() for c in range(n))


def expected(model, A, V):
    """(bytes, other_changed, outcome counts) lm_delta_map must give between the id sets A and V"""
    members, counts, undecided = {}, dict.fromkeys(OUTCOMES, 0), False
    for cid, keys in model.maps.items():
        upd, dele = {}, []
        for key in keys:
            wv = model.map_winner(cid, key, V)
            outcome, rep = classify(model.map_winner(cid, key, A), wv)
            if outcome in counts:
                counts[outcome] += 1
            if rep == "updated":
                upd[key] = shallow_json(wv)
                counts["new_child"] += isinstance(wv[3], wire.ContainerValue)
            elif rep == "deleted":
                dele.append(key)
            elif rep == "undecided":
                undecided = True
        if upd or dele:
            order = lambda k: k.encode("utf-8")
            members[to_json(cid_str(cid))] = '{"updated":{%s},"deleted":[%s]}' % (
                ",".join("%s:%s" % (to_json(k), upd[k]) for k in sorted(upd, key=order)), ",".join(to_json(k) for k in sorted(dele, key=order)))
    other = 0
    for ch in model.changes:
        for op in ch.ops:
            if op.cid.kind in (wire.KIND_MOVABLE, wire.KIND_TREE, wire.KIND_COUNTER):
                other |= any((ch.peer, op.counter + i) in V and (ch.peer, op.counter + i) not in A for i in range(op.atom_len))
    body = ",".join("%s:%s" % (k, members[k]) for k in sorted(members, key=lambda k: k.encode("utf-8")))
    return ("{" + body + "}").encode("utf-8"), (1 if other else 0) | (2 if undecided else 0), counts


def shallow_maps(model, X):
    """{ContainerID: {key: parsed shallow value}} of every Map at the id set X"""
    out = {}
    for cid, keys in model.maps.items():
        m = {}
        for key in keys:
            w = model.map_winner(cid, key, X)
            if w is not None and w[3] is not _GONE:
                m[key] = json.loads(shallow_json(w))
        out[cid_str(cid)] = m
    return out


def check_one(got, model, A, V, what=""):
    """one result (status, other_changed, bytes) against the reference: the bytes, then the applier"""
    want, oc, _ = expected(model, A, V)
    assert got[0] == OK, (what, got)
    assert got[2] == want, (what, got[2], want)
    assert got[1] == oc, (what, got[1], oc)
    delta = json.loads(got[2])
    at_a, at_v = shallow_maps(model, A), shallow_maps(model, V)
    for cid in at_v:
        m = dict(at_a[cid])
        d = delta.get(cid, {"updated": {}, "deleted": []})
        m.update(d["updated"])
        for k in d["deleted"]:
            m.pop(k, None)
        if oc & 2:        # keys the device did not decide are left out of the delta: they are left out of the comparison too
            skip = {k for k in at_v[cid] if k in at_a[cid] and k not in d["updated"] and _differs(at_a[cid][k], at_v[cid][k])}
            m = {k: v for k, v in m.items() if k not in skip}
            assert m == {k: v for k, v in at_v[cid].items() if k not in skip}, (what, cid)
        else:
            assert m == at_v[cid], (what, cid)
    assert set(delta) <= set(at_v), what


def _differs(a, b):
    return not (a == b) and isinstance(a, (list, dict)) and type(a) is type(b)


# ---- corpora: A = the empty version plus every recorded version, V = latest
def corpus_queries(docs, every=1):
    """[(document, frontiers of A)]: the empty version and every `every`-th recorded version of each document"""
    return [(i, fr) for i, d in enumerate(docs) for fr in [[]] + d.versions[::every]]


def corpus_counts(docs, queries):
    tot = dict.fromkeys(OUTCOMES, 0)
    for i, fr in queries:
        m = docs[i].model
        for k, v in expected(m, m.version(fr), m.all_ids)[2].items():
            tot[k] += v
    return tot


def check_conditions(name, docs, queries, at_least=AT_LEAST):
    tot = corpus_counts(docs, queries)
    for k, least in at_least.items():
        assert tot[k] >= least, (name, k, tot)
    return tot


def run_corpus(ctx, docs, queries, what="", fused=False):
    blobs = [d.blobs for d in docs]
    res = ctx.merge_batch(blobs)
    assert res == [d.model.result() for d in docs], what
    if fused:
        assert ctx.b.fused_documents(ctx.h) > 0, what
    got = ctx.delta_map([(i, docs[i].model.vv(fr)) for i, fr in queries])
    for (i, fr), g in zip(queries, got):
        m = docs[i].model
        check_one(g, m, m.version(fr), m.all_ids, (what, docs[i].label, fr))
    assert ctx.fetch() == res, what
    return len(queries)


# ---- hand cases: (name, replicas or (blobs, model), [(A as {peer: counter} or None, expected bytes, other_changed)])
def _root(body):
    return b'{"cid:root-m:Map":' + body + b"}"


def hand_cases():
    out = []
    R = wire.Replica
    r = R(5); r.map_set("m", "k", 1); r.commit()
    out.append(("A = V, A = empty", [r], [(dict(r.vv), b"{}", 0), (None, _root(b'{"updated":{"k":1},"deleted":[]}'), 0)]))
    r = R(6); r.map_set("m", "k", "s"); r.commit(); a = dict(r.vv)
    r.map_set("m", "k", "s"); r.commit()
    out.append(("set over set, an equal string", [r], [(a, b"{}", 0)]))
    r = R(7); r.map_set("m", "k", 3); r.map_set("m", "z", 0.0); r.map_set("m", "p", 1.0); r.map_set("m", "n", -0.0); r.commit(); a = dict(r.vv)
    r.map_set("m", "k", 3.0); r.map_set("m", "z", -0.0); r.map_set("m", "p", -0.0); r.map_set("m", "n", 1.0); r.commit()
    out.append(("3 against 3.0, 0.0 against -0.0, -0.0 against 1.0", [r], [(a, _root(b'{"updated":{"k":3.0,"n":1.0,"p":-0.0},"deleted":[]}'), 0)]))
    r = R(8); r.map_set("m", "k", 1); r.map_delete("m", "k"); r.map_set("m", "g", 1); r.commit(); a = dict(r.vv)
    r.map_delete("m", "k"); r.map_delete("m", "n"); r.map_delete("m", "g"); r.commit()
    out.append(("delete over delete, a key never written in A deleted in V", [r], [(a, _root(b'{"updated":{},"deleted":["g","n"]}'), 0)]))
    r = R(9); r.map_set("m", "same", b"\x00\xff"); r.map_set("m", "b", b"\x01"); r.commit(); a = dict(r.vv)
    r.map_set("m", "same", b"\x00\xff"); r.map_set("m", "b", b"\x01\x02"); r.map_set("m", "e", b""); r.commit()
    out.append(("binary values", [r], [(a, _root(b'{"updated":{"b":[1,2],"e":[]},"deleted":[]}'), 0)]))
    r = R(14); r.map_set("m", "x", 1); r.commit(); a = dict(r.vv)
    cm = r.map_set_container("m", "c", wire.KIND_MAP); r.map_set(cm, "in", 1)
    ct = r.map_set_container("m", "t", wire.KIND_TEXT); r.text_insert(ct, 0, "hey"); r.commit()
    want = ('{"cid:%d@14:Map":{"updated":{"in":1},"deleted":[]},"cid:root-m:Map":{"updated":{"c":"%s:cid:%d@14:Map","t":"%s:cid:%d@14:Text"},"deleted":[]}}'
            % (cm.counter, PARROT, cm.counter, PARROT, ct.counter)).encode("utf-8")
    out.append(("a child Map and a child Text created in V \\ A", [r], [(a, want, 0)]))
    r = R(15); cm = r.map_set_container("m", "k", wire.KIND_MAP); r.map_set(cm, "a", 1); r.commit(); a = dict(r.vv)
    r.map_set("m", "k", "plain"); r.map_set(cm, "b", 2); r.commit()
    want = ('{"cid:%d@15:Map":{"updated":{"b":2},"deleted":[]},"cid:root-m:Map":{"updated":{"k":"plain"},"deleted":[]}}' % cm.counter).encode()
    out.append(("a child Map hidden at V that still received writes", [r], [(a, want, 0)]))
    r = R(16); r.map_set("m", "k", [1, 2]); r.map_set("m", "q", {"a": 1}); r.commit(); a = dict(r.vv)
    r.map_set("m", "k", [1, 2]); r.map_set("m", "q", {"a": 1}); r.map_set("m", "j", 5); r.commit()
    out.append(("nested List over nested List, nested Map over nested Map, from other ops", [r], [(a, _root(b'{"updated":{"j":5},"deleted":[]}'), 2)]))
    r = R(17); r.map_set("m", "k", 1); r.map_set("m", "l", [1]); r.commit(); a = dict(r.vv)
    r.map_set("m", "k", {"b": [2], "a": 1}); r.map_set("m", "l", {"x": None}); r.commit()
    out.append(("a nested Map over a scalar and over a nested List", [r], [(a, _root(b'{"updated":{"k":{"a":1,"b":[2]},"l":{"x":null}},"deleted":[]}'), 0)]))
    r = R(18); r.map_set("m", "k", 1); r.commit(); a = dict(r.vv)
    r.mlist_insert("ml", 0, [1, 2]); r.map_set("m", "k", 2); r.commit(); a2 = dict(r.vv)
    r.text_insert("t", 0, "x"); r.list_insert("l", 0, [1]); r.commit()
    out.append(("a MovableList written next to a Map; Text and List ops set nothing", [r], [(a, _root(b'{"updated":{"k":2},"deleted":[]}'), 1), (a2, b"{}", 0)]))
    keys = ["", "\x01ctl", 'q"uote', "back\\slash", "ключ", "abcdefg", "abcdefgh", "abcdefgX", "L" * 300]
    r = R(19); r.map_set("m", "abcdefgh", 0); r.commit(); a = dict(r.vv)
    for i, k in enumerate(keys):
        r.map_set("m", k, i + 1)
    r.map_delete("m", "abcdefg"); r.map_delete("m", "\x01ctl"); r.commit()
    want = ('{"updated":{"":1,"%s":9,"abcdefgX":8,"abcdefgh":7,"back\\\\slash":4,"q\\"uote":3,"ключ":5},"deleted":["\\u0001ctl","abcdefg"]}' % ("L" * 300)).encode("utf-8")
    out.append(("keys: empty, 300 bytes, escapes, non-ASCII, a tie on the 8-byte prefix", [r], [(a, _root(want), 0)]))
    r = R(20); r.map_set("m", "k", 1); r.map_set("m", "k", 2); r.map_set("m", "j", 3); r.commit()
    out.append(("A cuts a change between two writes of one key", [r], [({20: 1}, _root(b'{"updated":{"j":3,"k":2},"deleted":[]}'), 0),
                                                                        ({20: 2}, _root(b'{"updated":{"j":3},"deleted":[]}'), 0)]))
    for lo, hi in (((1 << 32) - 1, 1 << 32), ((1 << 63) - 1, 1 << 63)):
        x, y = R(lo), R(hi)
        x.map_set("m", "k", "lo"); x.commit(); y.map_set("m", "k", "hi"); y.commit()
        out.append(("a lamport tie between peer ids %d and %d" % (lo, hi), [x, y], [({lo: 1}, _root(b'{"updated":{"k":"hi"},"deleted":[]}'), 0), ({hi: 1}, b"{}", 0),
                                                                                   (None, _root(b'{"updated":{"k":"hi"},"deleted":[]}'), 0)]))
    # a pending change delivered in V's blobs: c depends on b, whose blob is missing
    a_, b_, c_ = R(30), R(20), R(10)
    a_.map_set("m", "k", 1); a_.commit()
    b_.merge_from(a_); b_.map_set("m", "k", 2); b_.commit()
    c_.merge_from(b_); c_.map_set("m", "k", 3); c_.map_set("m", "only c", 4); c_.commit()
    blobs = [a_.export(), c_.export(dict(b_.vv))]
    model = _merge_ref.Model(changes_of([a_, b_, c_]), delivered=a_.changes[30] + c_.changes[10])
    assert model.pending == 2
    out.append(("a pending change delivered in V's blobs does not compete", (blobs, model), [(None, _root(b'{"updated":{"k":1},"deleted":[]}'), 0)]))
    r = R(21); r.map_set("m", "k", 1); r.commit(); a = dict(r.vv); first = r.export()
    r.map_set("m", "k", 2); r.commit()
    out.append(("a duplicated blob", ([first, r.export(), first, r.export()], _merge_ref.Model(changes_of([r]))), [(a, _root(b'{"updated":{"k":2},"deleted":[]}'), 0)]))
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
    got = ctx.delta_map(qs)
    for i, g, w in zip(info, got, want):
        assert g == w, (i[0], i[2], g, w)
    # … and the hand-written bytes agree with the derived reference
    for (name, d, a), w in zip(info, want):
        m = built[d][1]
        e = expected(m, vv_ids(a or {}), m.all_ids)
        assert (e[0], e[1]) == (w[2], w[1]), (name, e[:2], w)
    # statuses
    f = len(docs) - 1
    vv0 = res[0][2]
    peer, ctr = next(iter(_cursor.decode_vv(vv0).items()))
    enc = wire.encode_vv
    got = ctx.delta_map([(f, None), (0, enc({peer: ctr + 1})), (0, enc({peer: ctr, 424242: 1})), (0, enc({peer: ctr, 424242: 0})), (0, vv0[:-1]), (0, vv0 + b"\x00")])
    assert got[0][0] == res[-1][0] and got[0][2] == b""
    assert [g[0] for g in got[1:]] == [FRONTIERS_NOT_FOUND, FRONTIERS_NOT_FOUND, OK, DECODE_ERROR, DECODE_ERROR], got
    assert got[3][2] == b"{}"
    assert ctx.fetch() == res
    try:
        ctx.delta_map([(len(docs), None)])
    except RuntimeError:
        pass
    else:
        raise AssertionError("a call that cannot be answered must return -1")
    assert ctx.fetch() == res
    # lm_delta gives what it gave before lm_delta_map ran, and the other way round
    before = ctx.delta([(d, None) for d in range(len(cases))])
    assert ctx.delta_map(qs) == want and ctx.delta([(d, None) for d in range(len(cases))]) == before and ctx.fetch() == res


# ---- shapes
def slots_doc(n, peer=40):
    """`n` claimed slots: every key written at A, every key written again (every fifth deleted) in V \\ A, two keys more"""
    r = wire.Replica(peer)
    for i in range(n - 2):
        r.map_set("m", "k%03d" % i, 0)
    r.commit(); a = dict(r.vv)
    for i in range(n):
        if i % 5 == 4:
            r.map_delete("m", "k%03d" % i)
        else:
            r.map_set("m", "k%03d" % i, 0 if i % 7 == 0 else i)
    r.commit()
    assert len(r.changes[peer][0].ops) + len(r.changes[peer][1].ops) == 2 * n - 2
    return r, a


def rows_doc(n, peer=41):
    """`n` op rows on seven keys"""
    r = wire.Replica(peer)
    for i in range(n):
        r.map_set("m", "k%d" % (i % 7), i)
        if i == n // 2:
            r.commit(); a = dict(r.vv)
    r.commit()
    return r, a


def run_shapes(ctx):
    """63 / 64 / 65 / 129 claimed slots and op rows; a document without Map rows between two with; several A on one document"""
    reps = [slots_doc(n, 400 + n) for n in (63, 64, 65, 129)] + [rows_doc(n, 600 + n) for n in (63, 64, 65, 129)]
    t = wire.Replica(77); t.text_insert("t", 0, "no map here"); t.commit()
    docs = [[r.export()] for r, _ in reps]
    docs.insert(3, [t.export()])
    models = [_merge_ref.Model(changes_of([r])) for r, _ in reps]
    models.insert(3, _merge_ref.Model(changes_of([t])))
    avv = [a for _, a in reps]
    avv.insert(3, dict(t.vv))
    res = ctx.merge_batch(docs)
    assert res == [m.result() for m in models]
    qs = [(d, a) for d in range(len(docs)) for a in (avv[d], None)] + [(0, {463: k}) for k in (1, 30, 61, 62, 100)]
    got = ctx.delta_map([(d, None if a is None else wire.encode_vv(a)) for d, a in qs])
    for (d, a), g in zip(qs, got):
        check_one(g, models[d], vv_ids(a or {}), models[d].all_ids, ("shapes", d, a))
    assert got[6][2] == b"{}" and got[7][2] == b"{}" and got[0][2] != b"{}"
    assert ctx.fetch() == res


def run_tables(ctx, ht_opt=None, what=""):
    """distinct pairs one below, at and one above half the largest LDS table (the LDS / HBM builder switch), from the empty version and
    from the first peer's end"""
    n = 0
    for label, _, docs in _merge_docs_map.table_docs(ht_opt):
        d = docs[0]
        res = ctx.merge_batch([d.blobs])
        assert res == [d.model.result()], (what, label)
        first = d.reps[0]
        qs = [None, {first.peer: first.vv[first.peer]}]
        got = ctx.delta_map([(0, None if a is None else wire.encode_vv(a)) for a in qs])
        for a, g in zip(qs, got):
            check_one(g, d.model, vv_ids(a or {}), d.model.all_ids, (what, label, a))
        assert ctx.fetch() == res
        n += 1
    return n


def run_overflow(ctx):
    """400 keys of 200-byte string values from the empty version: the answer is larger than the optimistic slab"""
    r = wire.Replica(51)
    for i in range(400):
        r.map_set("m", "k%03d" % i, ("%03d" % i) * 66 + "xy")
    r.commit()
    m = _merge_ref.Model(changes_of([r]))
    want, _, _ = expected(m, frozenset(), m.all_ids)
    ctx.set_profiling(1)
    res = ctx.merge_batch([[r.export()]])
    assert len(want) > len(res[0][1]) > 400 * 200
    check_one(ctx.delta_map([(0, None)])[0], m, frozenset(), m.all_ids, "slab overflow")
    assert ctx.b.delta_bytes(ctx.h) == ((len(want) + 15) & ~15) + 2 * 16                 # the bytes written + a result row per launch
    assert [n for n, _ in ctx.kernel_times()].count("k_mdelta") == 2                      # the second launch, at exact sizes
    ctx.set_profiling(0)
    assert ctx.fetch() == res


def run_bytes_moved(ctx):
    """what crosses to the host is proportional to the change: one changed key in a 1,000-key Map copies back under 256 bytes"""
    r = wire.Replica(52)
    for i in range(1000):
        r.map_set("m", "key%04d" % i, i)
    r.commit(); a = dict(r.vv)
    r.map_set("m", "key0500", "changed"); r.commit()
    res = ctx.merge_batch([[r.export()]])
    assert len(res[0][1]) > 12000
    want = b'{"cid:root-m:Map":{"updated":{"key0500":"changed"},"deleted":[]}}'
    assert ctx.delta_map([(0, wire.encode_vv(a))]) == [(OK, 0, want)]
    assert ctx.b.delta_bytes(ctx.h) == ((len(want) + 15) & ~15) + 16 < 256
    assert ctx.fetch() == res


def steps(seed=5):
    """a two-writer Map history exported at three versions of the first writer: (export, frontiers, vv) each"""
    import random
    rng = random.Random(seed)
    r, o = wire.Replica(31), wire.Replica(32)
    for i in range(30):
        o.map_set("m", "k%d" % rng.randrange(6), "o%d" % i)
    o.commit()
    out = []
    for s in range(3):
        for _ in range(40):
            k = "k%d" % rng.randrange(8)
            if rng.random() < 0.25:
                r.map_delete("m", k)
            else:
                r.map_set("m", k, rng.choice([1, 2, "s", 2.5, None]))
            if rng.random() < 0.3:
                r.commit()
        r.commit()
        if s == 0:
            r.merge_from(o)
        out.append((r.export(), list(r.frontiers), dict(r.vv)))
    return out, _merge_ref.Model(changes_of([r]))


def run_checkout(ctx):
    ((_, _, v1), (_, f2, v2), (e3, _, v3)), model = steps()
    docs, fronts = [[e3], [e3]], [wire.encode_frontiers(f2), None]
    res = ctx.merge_batch(docs, fronts)
    assert res == [model.result(f2), model.result()]
    got = ctx.delta_map([(0, wire.encode_vv(v1)), (1, wire.encode_vv(v1)), (0, wire.encode_vv(v2)), (0, wire.encode_vv(v3)), (1, wire.encode_vv(v2))])
    check_one(got[0], model, vv_ids(v1), model.version(f2), "checkout")
    check_one(got[1], model, vv_ids(v1), model.all_ids, "latest next to it")
    assert got[2][0] == OK and got[2][2] == b"{}"
    assert got[3][0] == FRONTIERS_NOT_FOUND                                  # A beyond the rendered version
    check_one(got[4], model, vv_ids(v2), model.all_ids, "latest from the checkout's version")
    assert got[0][2] != b"{}" and got[4][2] != b"{}"
    assert ctx.fetch() == res


def resident_flow(ctx, n_docs=6):
    """stage + run, keep vv1 from fetch(); import_more + run, delta_map(from vv1); a third step with A = vv1 and A = vv2"""
    import random
    reps, firsts, seconds, thirds, vv1m, vv2m = [], [], [], [], [], []
    for s in range(n_docs):
        rng = random.Random(900 + s)
        a, b = wire.Replica(7000 + s), wire.Replica(8000 + s)

        def write(r, n):
            for _ in range(n):
                k = "k%d" % rng.randrange(9)
                if rng.random() < 0.2:
                    r.map_delete("m", k)
                else:
                    r.map_set("m", k, rng.choice([rng.randrange(5), "v", 1.5, None, True]))
                if rng.random() < 0.3:
                    r.commit()
            r.commit()
        write(a, 30); write(b, 20)
        firsts.append([a.export(), b.export()]); have = (dict(a.vv), dict(b.vv)); vv1m.append({**a.vv, **b.vv})
        a.merge_from(b); write(a, 25)
        seconds.append([a.export(vv1m[-1])]); vv2m.append(dict(a.vv))
        write(b, 15)
        thirds.append([b.export(have[1])])
        a.merge_from(b)
        reps.append(a)
    ctx.stage(firsts); ctx.run()
    r1 = ctx.fetch()
    vv1 = [r[2] for r in r1]
    assert vv1 == [wire.encode_vv(v) for v in vv1m]
    ctx.import_more(seconds); ctx.run()
    r2 = ctx.fetch()
    models = [_merge_ref.Model(changes_of([r])) for r in reps]
    got = ctx.delta_map([(d, vv1[d]) for d in range(n_docs)])
    for d, g in enumerate(got):
        check_one(g, models[d], vv_ids(vv1m[d]), vv_ids(vv2m[d]), ("resident", d))
        assert g[2] != b"{}"
    assert ctx.fetch() == r2
    ctx.import_more(thirds); ctx.run()
    r3 = ctx.fetch()
    got = ctx.delta_map([(d, vv1[d]) for d in range(n_docs)] + [(d, r2[d][2]) for d in range(n_docs)])
    for d in range(n_docs):
        check_one(got[d], models[d], vv_ids(vv1m[d]), models[d].all_ids, ("resident, two imports back", d))
        check_one(got[n_docs + d], models[d], vv_ids(vv2m[d]), models[d].all_ids, ("resident, one import back", d))
    assert ctx.fetch() == r3


def run_self_check(ctx, monkeypatch):
    """the self-check is the call's safety argument: with LM_DELTA_SKEW the device is handed an empty V, no row competes, the winner at V
    found from the op rows differs from the table's for every key — every query on a document with a Map write must come back
    LM_UNSUPPORTED with no bytes, also one whose A equals V; without the knob the same queries are answered"""
    docs = []
    for seed in range(5000, 5006):
        reps, versions = _merge_docs_map.map_session(seed, 3, n_steps=40)
        docs.append(_merge_docs_map.MapDoc("seed %d" % seed, reps, versions=versions))
    res = ctx.merge_batch([d.blobs for d in docs])
    q = [(i, d.model.vv(fr)) for i, d in enumerate(docs) for fr in ([], None)]
    good = ctx.delta_map(q)
    assert all(g[0] == OK for g in good) and all(g[2] != b"{}" for g in good[::2]) and all(g[2] == b"{}" for g in good[1::2])
    monkeypatch.setenv("LM_DELTA_SKEW", "1")
    assert ctx.delta_map(q) == [(UNSUPPORTED, 0, b"")] * len(q)
    monkeypatch.delenv("LM_DELTA_SKEW")
    assert ctx.delta_map(q) == good and ctx.fetch() == res


def run_snapshot(ctx):
    """a snapshot staged from its state section: the call stages it once more through its history (lm_delta's batch shapes)"""
    import _oracle
    reps, versions = _merge_docs_map.map_session(4100, 3, n_steps=80)
    d = _merge_docs_map.MapDoc("snapshot", reps, versions=versions)
    full = wire.Replica(reps[0].peer)
    for r in reps:
        full.merge_from(r)
    st, ents = _oracle.state_entries([full.export()])
    assert st == 0
    res = ctx.merge_batch([[full.export_snapshot(state=ents)]])
    assert ctx.b.state_documents(ctx.h) == 1 and res[0][:2] == d.model.result()[:2]
    frs = [[]] + d.versions[:6]
    got = ctx.delta_map([(0, d.model.vv(fr)) for fr in frs])
    for fr, g in zip(frs, got):
        check_one(g, d.model, d.model.version(fr), d.model.all_ids, ("state-staged snapshot", fr))
    assert got[0][2] != b"{}"
    assert ctx.fetch() == res
