"""Text / List deltas between two versions (lm_delta) restated over the PLAIN merge model (tests/_merge_ref.py): the expected
answers at any pair of versions, the corpora, and the documents built on the boundaries of k_delta_mark / k_delta, shared by
test_delta_ref.py (kernel-logic harness) and test_gpu_zz_delta_ref.py (device).  The expectation is the model's alone: no oracle,
kernel or decoder code, nothing of _delta.expected (only the ~20-line applier `_delta.apply` is used, as the form-independent check).

The statement (include/loro_merge.h, "Text and List deltas between two versions").  A and V are SETS of ids: V = Model.version(the
rendered frontiers), A = Model.version(frontiers) or, for a version vector, {(p, c) : c < A[p]} — causally closed or not.  For every
Text / List key of `model.seqs`, root or child, take `model.seqs[cid]`, the elements in sequence order:
  * an element is in X iff `_merge_ref._visible(e, X)`: its id is in X and no delete atom whose own id is in X hit it;
  * a Text element whose `what[0]` is not "char" (a style anchor) is no element;
  * K = in A and in V, I = in V only, D = in A only, anything else is skipped;
  * a maximal run of K: {"retain":n}; the I and D between two K runs (or a container edge): at most one {"insert":…} with every I in
    sequence order, then at most one {"delete":n}; a trailing retain is dropped; an empty delta leaves the container out;
  * units == 1: a Text retain / delete counts 2 for a scalar >= U+10000;
  * a Text insert is the scalars escaped by `escape` (below); a List insert the values by `_values.to_json`; a value that is a child
    container is the JSON string U+1F99C ":cid:<counter>@<peer>:<Kind>" from the ELEMENT's own id;
  * the members in the bytewise order of their JSON-encoded keys;
  * other_changed = 1 iff an op of a container that is neither Text nor List (Map, MovableList) has an atom id in V \\ A — from the
    model's changes, atom by atom, so an A that cuts inside a MovableList insert row counts;
  * some A[p] > V[p]: LM_FRONTIERS_NOT_FOUND, no bytes.

Floors (FLOORS), asserted from the model before anything is compared, with the counts seen over RICH_SEEDS = 900..929 and
NESTED_SEEDS = 950..979 — every recorded version once as V (1,559 entries); per V the empty version, at most eight recorded A's inside
V chosen by a seeded rule that prefers multi-head A's, the version in front of a head's trailing Map ops, and one version vector that
is not causally closed: 12,697 (A, V) pairs, 12,078 of them with V not the latest:
  child_text_all_three 200 (1,445), child_list_all_three 200 (1,228), root_list_all_three 200 (3,764), insert_behind_delete 500
  (11,703), inserted_children 500 (19,013), astral_kept_or_deleted 200 (9,323), multi_head_a 50 (485), multi_head_v 50 (60),
  empty_other_1 100 (251), empty_other_0 100 (1,163), one_of_two_deleters_in_a 100 (5,865), open_vector_a 50 (1,305)."""
import json
import random

import _cursor_ref, _delta, _merge_docs, _merge_ref
from _cursor_ref import Doc, cid_str, EDGE_PEERS
from _delta import OK, UNSUPPORTED, FRONTIERS_NOT_FOUND
from _merge_ref import _visible
from _values import to_json
from loro_amd import wire

SEQ = (wire.KIND_TEXT, wire.KIND_LIST)
ASTRAL = "\U0001F600"
RICH_SEEDS, NESTED_SEEDS = range(900, 930), range(950, 980)
FLOORS = {"child_text_all_three": 200, "child_list_all_three": 200, "root_list_all_three": 200, "insert_behind_delete": 500,
          "inserted_children": 500, "astral_kept_or_deleted": 200, "multi_head_a": 50, "multi_head_v": 50, "empty_other_1": 100,
          "empty_other_0": 100, "one_of_two_deleters_in_a": 100, "open_vector_a": 50}


# ------------------------------------------------------------------------------------------------------------------- the statement
_SHORT = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\f": "\\f", "\n": "\\n", "\r": "\\r", "\t": "\\t"}


def escape(ch):
    """one scalar as the JSON of a Text value holds it: the short escapes, \\u00XX for the other control characters, else itself"""
    if ch in _SHORT:
        return _SHORT[ch]
    return "\\u%04x" % ord(ch) if ord(ch) < 0x20 else ch


def vector_ids(vv):
    """the id set of a version vector {peer: end}"""
    return frozenset((p, c) for p, n in vv.items() for c in range(n))


def vector_of(ids):
    out = {}
    for p, c in ids:
        out[p] = max(out.get(p, 0), c + 1)
    return out


def piece(e):
    """the payload text of one inserted List element"""
    v = e.what[1]
    if isinstance(v, wire.ContainerValue):
        return to_json("\U0001F99C:cid:%d@%d:%s" % (e.id[1], e.id[0], _cursor_ref.KIND_NAME[v.kind]))
    return to_json(v)


def classes(model, cid, A, V):
    """[(class, element)] of one container in sequence order, class in "KID" """
    text = cid.kind == wire.KIND_TEXT
    out = []
    for e in model.seqs[cid]:
        if text and e.what[0] != "char":
            continue
        a, v = _visible(e, A), _visible(e, V)
        if a or v:
            out.append(("K" if a and v else "I" if v else "D", e))
    return out


def container_ops(model, cid, A, V, units, counts=None):
    """the canonical delta of one container: [("retain", n) | ("insert", [payload pieces]) | ("delete", n)]"""
    text = cid.kind == wire.KIND_TEXT
    ops, retain, ins, dele, seen_d, behind = [], 0, [], 0, False, False

    def width(e):
        return 2 if text and units == 1 and ord(e.what[1]) >= 0x10000 else 1
    for k, e in classes(model, cid, A, V) + [("K", None)]:
        if k == "K":
            if ins:
                ops.append(("insert", ins))
            if dele:
                ops.append(("delete", dele))
            if counts is not None and behind:
                counts["insert_behind_delete"] += 1
            ins, dele, seen_d, behind = [], 0, False, False
            if e is not None:
                if ops and ops[-1][0] == "retain":
                    ops[-1] = ("retain", ops[-1][1] + width(e))
                else:
                    ops.append(("retain", width(e)))
        else:
            if k == "I":
                ins.append(escape(e.what[1]) if text else piece(e))
                behind |= seen_d
                if counts is not None and not text and isinstance(e.what[1], wire.ContainerValue):
                    counts["inserted_children"] += 1
            else:
                dele += width(e)
                seen_d = True
        if counts is not None and e is not None:
            if k != "I" and text and ord(e.what[1]) >= 0x10000:
                counts["astral_kept_or_deleted"] += 1
    if ops and ops[-1][0] == "retain":
        ops.pop()
    return ops


def op_text(ops, text):
    out = []
    for k, v in ops:
        if k == "insert":
            out.append('{"insert":"%s"}' % "".join(v) if text else '{"insert":[%s]}' % ",".join(v))
        else:
            out.append('{"%s":%d}' % (k, v))
    return "[" + ",".join(out) + "]"


def other_changed(model, A, V):
    for ch in model.changes:
        for op in ch.ops:
            if op.cid.kind not in SEQ and any((ch.peer, op.counter + i) in V and (ch.peer, op.counter + i) not in A for i in range(op.atom_len)):
                return 1
    return 0


def sequence_cids(model):
    return [c for c in model.seqs if c.kind in SEQ]


class Expect:
    """what lm_delta must give for one (A, V, units): .status, .other, .bytes, .ops {key: ops}"""

    def __init__(self, model, A, V, units=0, counts=None):
        self.model, self.A, self.V, self.units = model, A, V, units
        va, vv = vector_of(A), vector_of(V)
        if any(n > vv.get(p, 0) for p, n in va.items()):
            self.status, self.other, self.bytes, self.ops = FRONTIERS_NOT_FOUND, 0, b"", {}
            return
        self.ops = {}
        for cid in sequence_cids(model):
            ops = container_ops(model, cid, A, V, units, counts)
            if counts is not None:         # (such an element is in neither version: no class, counted here)
                counts["one_of_two_deleters_in_a"] += sum(1 for e in model.seqs[cid] if len(e.deleters) >= 2 and e.id in A and sum(1 for x in e.deleters if x in A) == 1
                                                          and sum(1 for x in e.deleters if x in V) >= 2)
            if ops:
                self.ops[cid] = ops
                if counts is not None and {k for k, _ in ops} == {"retain", "insert", "delete"}:
                    name = ("root_" if cid.root else "child_") + ("text" if cid.kind == wire.KIND_TEXT else "list") + "_all_three"
                    counts[name] = counts.get(name, 0) + 1
        members = {to_json(cid_str(c)): op_text(o, c.kind == wire.KIND_TEXT) for c, o in self.ops.items()}
        body = ",".join("%s:%s" % (k, members[k]) for k in sorted(members, key=lambda k: k.encode("utf-8")))
        self.status, self.other, self.bytes = OK, other_changed(model, A, V), ("{" + body + "}").encode("utf-8")
        if counts is not None:
            counts["empty_other_%d" % self.other] += not self.ops

    def answer(self):
        return (self.status, self.other, self.bytes)


def value_at(model, cid, X):
    """a container's value at the id set X as json.loads gives it back: a Text's string, a List's values (a child as its parrot string)"""
    if cid.kind == wire.KIND_TEXT:
        return "".join(e.what[1] for e in model.seqs[cid] if e.what[0] == "char" and _visible(e, X))
    return [json.loads(piece(e)) for e in model.seqs[cid] if _visible(e, X)]


def check_one(got, ex, what=""):
    """one result (status, other_changed, bytes) against the statement: all three, then the applier per container"""
    assert got[0] == ex.status, (what, got, ex.answer())
    assert got[2] == ex.bytes, (what, got[2], ex.bytes)
    assert got[1] == ex.other, (what, got[1], ex.other)
    if ex.status == OK:
        check_applies(json.loads(got[2]), ex, what)


def check_applies(delta, ex, what=""):
    """form-independent: the ops take the model's value at A to the model's value at V, per container"""
    keys = {cid_str(c): c for c in sequence_cids(ex.model)}
    assert set(delta) <= set(keys), what
    for key, cid in keys.items():
        assert _delta.apply(value_at(ex.model, cid, ex.A), delta.get(key, []), ex.units) == value_at(ex.model, cid, ex.V), (what, key)


# -------------------------------------------------------------------------------------------------------------------- the corpora
class Entry:
    """one batch entry: a document rendered at one version V, and the A's asked of it: [(label, id set, vv bytes or None)]"""

    def __init__(self, doc, label, frontiers):
        self.doc, self.label, self.frontiers = doc, "%s at %s" % (doc.label, label), frontiers
        self.V = doc.model.version(frontiers)
        self.asks = []

    def ask(self, label, A, vv_bytes="derive"):
        self.asks.append((label, A, wire.encode_vv(vector_of(A)) if vv_bytes == "derive" else vv_bytes))


def open_vector(model, V, rng):
    """a version vector inside V whose id set is NOT causally closed (it holds an id and lacks one of that id's causes), or None"""
    vv = vector_of(V)
    for _ in range(30):
        cut = {p: rng.randint(0, n) for p, n in vv.items()}
        A = vector_ids(cut)
        if any(not model.closure_of_id(max((i for i in A if i[0] == p), key=lambda i: i[1])) <= A for p, n in cut.items() if n):
            return A
    return None


def before_trailing_other_ops(model, V, frontiers):
    """V without the atoms of Map / MovableList ops that end one of its heads (the head whose run of such atoms is longest), or None
    when every head of V ends in a Text / List op: from there to V the delta is {} and other_changed is 1"""
    kind = getattr(model, "_delta_ref_kind", None)
    if kind is None:
        kind = model._delta_ref_kind = {(ch.peer, op.counter + i): op.cid.kind for ch in model.changes for op in ch.ops for i in range(op.atom_len)}
    heads = frontiers if frontiers is not None else [(p, n - 1) for p, n in vector_of(V).items()]
    best = frozenset()
    for p, c in heads:
        tail = set()
        while c >= 0 and kind[(p, c)] not in SEQ:
            tail.add((p, c)); c -= 1
        if len(tail) > len(best):
            best = frozenset(tail)
    return V - best if best else None


def entries_of(docs, every=1, max_a=8):
    """every version of every `every`-th document as V; per V the empty version, at most `max_a` recorded versions inside V (multi-head
    ones first, the rest by a seeded shuffle) and one open vector -> ([Entry], counts of the choice)"""
    out, counts = [], {"multi_head_a": 0, "multi_head_v": 0, "open_vector_a": 0, "v_not_latest": 0, "pairs": 0}
    for d in docs[::every]:
        sets = [(label, fr, d.model.version(fr)) for label, fr in d.versions]
        for k, (label, fr, V) in enumerate(sets):
            rng = random.Random("%s/%d" % (d.label, k))
            e = Entry(d, label, fr)
            e.ask("empty", frozenset(), None)
            inside = [(l, f, X) for l, f, X in sets if X <= V]
            rng.shuffle(inside)
            inside.sort(key=lambda x: not (x[1] is not None and len(x[1]) > 1))          # (stable: multi-head first)
            for l, f, X in inside[:max_a]:
                e.ask(l, X)
                counts["multi_head_a"] += f is not None and len(f) > 1
            A = before_trailing_other_ops(d.model, V, fr)
            if A is not None:
                e.ask("in front of the trailing Map ops", A)
            A = open_vector(d.model, V, rng)
            if A is not None:
                e.ask("open vector", A)
                counts["open_vector_a"] += 1
            counts["multi_head_v"] += fr is not None and len(fr) > 1
            counts["v_not_latest"] += (V != d.model.all_ids) * len(e.asks)
            counts["pairs"] += len(e.asks)
            out.append(e)
    return out, counts


def expectations(entries, counts=None):
    """{units: [[Expect per ask] per entry]}; `counts`: the floors' counts, summed over units == 0"""
    out = {}
    for units in (0, 1):
        out[units] = [[Expect(e.doc.model, A, e.V, units, counts if units == 0 else None) for _, A, _ in e.asks] for e in entries]
    return out


def new_counts():
    return dict.fromkeys(FLOORS, 0)


def check_floors(counts, floors=FLOORS):
    for k, least in floors.items():
        assert counts[k] >= least, (k, counts)


def run_entries(ctx, entries, want, what="", units=(0, 1)):
    """the entries as one batch (each at its checkout), every ask in one call per units -> queries compared.  Every query on these
    legal documents must come back as the statement says: no LM_UNSUPPORTED is allowed"""
    blobs = [e.doc.blobs for e in entries]
    fronts = [None if e.frontiers is None else wire.encode_frontiers(e.frontiers) for e in entries]
    res = ctx.merge_batch(blobs, fronts if any(f is not None for f in fronts) else None)
    assert res == [e.doc.model.result(e.frontiers) for e in entries], what
    n = run_asks(ctx, entries, want, what, units)
    assert ctx.fetch() == res, what
    return n


def run_asks(ctx, entries, want, what="", units=(0, 1), order=None):
    qs = [(k, j) for k, e in enumerate(entries) for j in range(len(e.asks))]
    if order is not None:
        random.Random(order).shuffle(qs)
    for u in units:
        got = ctx.delta([(k, entries[k].asks[j][2]) for k, j in qs], u)
        assert not [g for g in got if g[0] == UNSUPPORTED], (what, "a refusal on a legal document")
        for (k, j), g in zip(qs, got):
            check_one(g, want[u][k][j], (what, entries[k].label, entries[k].asks[j][0], u))
    return len(qs) * len(units)


def run_resident(ctx, docs, what="resident"):
    """`docs` resident; every version by an import that brings nothing; asked from the version stood at before and from the empty one"""
    ctx.stage([d.blobs for d in docs]); ctx.run()
    n = 0
    prev = [frozenset()] * len(docs)
    for v in range(max(len(d.versions) for d in docs)):
        frs = [d.versions[v][1] if v < len(d.versions) else None for d in docs]
        if v:
            ctx.import_more([[] for _ in docs], [None if fr is None else wire.encode_frontiers(fr) for fr in frs]); ctx.run()
        res = ctx.fetch()
        Vs = [d.model.version(fr) for d, fr in zip(docs, frs)]
        for u in (0, 1):
            qs, exs = [], []
            for i, d in enumerate(docs):
                for A in (prev[i], frozenset()):
                    qs.append((i, wire.encode_vv(vector_of(A)) if A else None)); exs.append(Expect(d.model, A, Vs[i], u))
            got = ctx.delta(qs, u)
            for q, g, ex in zip(qs, got, exs):
                check_one(g, ex, (what, docs[q[0]].label, v, u))
            n += len(qs)
        assert ctx.fetch() == res
        prev = Vs
    return n


def run_steps(ctx, docs, what="steps"):
    """the sessions of _cursor_ref.step_docs: after every step, at both versions it stands at, asked from the vv of the step before
    and from the empty version -> queries compared"""
    n = len(docs[0].steps)
    ws = [d.wire_steps() for d in docs]
    sessions = [_merge_ref.Session(d.changes) for d in docs]
    prev = [frozenset()] * len(docs)
    total = 0
    for k in range(n):
        blobs = [w[k][0] for w in ws]
        if k == 0:
            ctx.stage(blobs, None)
            ctx.import_more([[] for _ in docs], None)
        else:
            ctx.import_more(blobs, None)
        ctx.run()
        want = [s.step([c for _, cs in d.steps[k][0] for c in cs], None) for s, d in zip(sessions, docs)]
        frs = [d.steps[k][1] for d in docs]
        for sub in (0, 1):
            if sub:
                if not any(fr is not None for fr in frs):
                    break
                ctx.import_more([[] for _ in docs], [None if fr is None else wire.encode_frontiers(fr) for fr in frs])
                ctx.run()
                want = [s.step([], fr) for s, fr in zip(sessions, frs)]
            got = ctx.fetch()
            for d, g, w in zip(docs, got, want):
                assert g == w, (what, d.label, k, sub, g, w)
            qs, exs = [], []
            for i, s in enumerate(sessions):
                if sub and frs[i] is None:
                    continue
                V = s.model.version(frs[i] if sub else None)
                for A in (prev[i], frozenset()):
                    qs.append((i, wire.encode_vv(vector_of(A)) if A else None)); exs.append(Expect(s.model, A, V, k & 1))
            res = ctx.delta(qs, k & 1)
            for q, g, ex in zip(qs, res, exs):
                check_one(g, ex, (what, docs[q[0]].label, k, sub))
            total += len(qs)
        prev = [s.model.all_ids for s in sessions]
    return total


# ------------------------------------------------------------------------------- the hand-written answers, for the statement's test
def recorded(build):
    """build() with every export of a wire.Replica recorded -> (its result, {blob: the changes its replica held at that export}).
    _delta.hand_cases() hands out blobs only and stays as it is; the model needs the writers' Change objects, and several cases export
    one replica at more than one version, so the changes are taken at the moment of each export.  `wire.Replica` is swapped for the
    time of the call only: a builder that holds its own reference to the class (`from loro_amd.wire import Replica`) is not recorded,
    and hand_models() then fails with a KeyError on the blob, not silently"""
    exports, plain = {}, wire.Replica

    class Recorded(plain):
        def export(self, *a, **kw):
            blob = plain.export(self, *a, **kw)
            if not a and not kw:
                exports[blob] = [c for cs in self.changes.values() for c in cs]
            return blob
    wire.Replica = Recorded
    try:
        out = build()
    finally:
        wire.Replica = plain
    return out, exports


def hand_models():
    """[(name, model of V, id set A, {units: bytes}, other_changed)] of _delta.hand_cases().  The cases hand out blobs only: the
    changes behind a blob are what its replica held when it exported it (recorded while the cases are built)"""
    cases, exports = recorded(_delta.hand_cases)
    out = []
    for name, blobs, a_blobs, exp, oc in cases:
        model = _merge_ref.Model(exports[blobs[0]])
        A = frozenset() if a_blobs is None else frozenset((c.peer, k) for c in exports[a_blobs[0]] for k in range(c.counter, c.ctr_end))
        out.append((name, model, A, exp, oc))
    return out


def _doc(label, peer, build, versions=()):
    r = wire.Replica(peer)
    got = build(r)
    r.commit()
    return Doc(label, [r], versions), got


def literals():
    """about 30 answers written out by hand: [(name, Doc, A as {peer: end}, frontiers of V or None, {units: bytes}, other_changed)];
    bytes None = LM_FRONTIERS_NOT_FOUND"""
    T, L = '"cid:root-text:Text":', '"cid:root-list:List":'
    out = []

    def add(name, peer, build, a, exp, oc=0, v=None):
        d, _ = _doc(name, peer, build)
        out.append((name, d, a, v, {u: None if e is None else ("{" + e + "}").encode("utf-8") for u, e in exp.items()}, oc))
    add("insert at the front", 101, lambda r: (r.text_insert("text", 0, "bc"), r.commit(), r.text_insert("text", 0, "a")), {101: 2}, {0: T + '[{"insert":"a"}]'})
    add("insert in the middle", 102, lambda r: (r.text_insert("text", 0, "ac"), r.commit(), r.text_insert("text", 1, "b")), {102: 2}, {0: T + '[{"retain":1},{"insert":"b"}]'})
    add("delete at the front", 103, lambda r: (r.text_insert("text", 0, "abc"), r.commit(), r.text_delete("text", 0, 1)), {103: 3}, {0: T + '[{"delete":1}]'})
    add("delete at the end: the retain in front stays", 104, lambda r: (r.text_insert("text", 0, "abc"), r.commit(), r.text_delete("text", 2, 1)), {104: 3},
        {0: T + '[{"retain":2},{"delete":1}]'})
    add("insert then delete at one place: insert first", 105, lambda r: (r.text_insert("text", 0, "abc"), r.commit(), r.text_delete("text", 1, 1), r.text_insert("text", 1, "XY")),
        {105: 3}, {0: T + '[{"retain":1},{"insert":"XY"},{"delete":1}]'})
    # a b c d -> a X [b] Y [c] d: X stands in front of b, Y between the tombstones: ONE insert "XY", one delete 2
    add("two inserts around two deletes join", 106, lambda r: (r.text_insert("text", 0, "abcd"), r.commit(), r.text_insert("text", 1, "X"), r.text_insert("text", 3, "Y"),
                                                                r.text_delete("text", 2, 1), r.text_delete("text", 3, 1)),
        {106: 4}, {0: T + '[{"retain":1},{"insert":"XY"},{"delete":2}]'})
    add("typed and deleted between A and V: skipped", 107, lambda r: (r.text_insert("text", 0, "ab"), r.commit(), r.text_insert("text", 1, "zzz"), r.text_delete("text", 1, 3)),
        {107: 2}, {0: ""})
    add("typed and deleted, with a survivor", 108, lambda r: (r.text_insert("text", 0, "ab"), r.commit(), r.text_insert("text", 1, "xyz"), r.text_delete("text", 2, 1)),
        {108: 2}, {0: T + '[{"retain":1},{"insert":"xz"}]'})
    add("A inside an insert op", 109, lambda r: r.text_insert("text", 0, "hello"), {109: 2}, {0: T + '[{"retain":2},{"insert":"llo"}]'})
    add("A inside a delete op", 110, lambda r: (r.text_insert("text", 0, "abcdef"), r.text_delete("text", 1, 4)), {110: 8}, {0: T + '[{"retain":1},{"delete":2}]'})
    add("astral kept, deleted and inserted", 111, lambda r: (r.text_insert("text", 0, ASTRAL + "a" + ASTRAL), r.commit(), r.text_delete("text", 2, 1), r.text_insert("text", 2, ASTRAL + "b")),
        {111: 3}, {0: T + '[{"retain":2},{"insert":"%sb"},{"delete":1}]' % ASTRAL, 1: T + '[{"retain":3},{"insert":"%sb"},{"delete":2}]' % ASTRAL})
    add("astral as the last scalar of a retain", 112, lambda r: (r.text_insert("text", 0, "a" + ASTRAL), r.commit(), r.text_insert("text", 2, "!")),
        {112: 2}, {0: T + '[{"retain":2},{"insert":"!"}]', 1: T + '[{"retain":3},{"insert":"!"}]'})
    add("every short escape and two long ones", 113, lambda r: r.text_insert("text", 0, "\"\\\b\f\n\r\t\x00\x1f\x7f/"), {},
        {0: T + '[{"insert":"\\"\\\\\\b\\f\\n\\r\\t\\u0000\\u001f\x7f/"}]'})
    add("2-, 3- and 4-byte scalars", 114, lambda r: r.text_insert("text", 0, "é中" + ASTRAL), {}, {0: T + '[{"insert":"é中%s"}]' % ASTRAL})
    add("only a style mark added", 115, lambda r: (r.text_insert("text", 0, "abcd"), r.commit(), r.text_mark("text", 1, 3, "bold", True)), {115: 4}, {0: ""})
    add("only an anchor deleted", 116, lambda r: (r.text_insert("text", 0, "abcd"), r.text_mark("text", 1, 3, "bold", True), r.text_delete("text", 2, 1), r.commit(), r.text_delete("text", 1, 1)),
        {116: 7}, {0: ""})                     # entities a S b c E d: entity 2 (b) goes below A; entity 1 (S) after it
    add("only a trailing retain", 117, lambda r: (r.text_insert("text", 0, "abcd"), r.commit(), r.list_insert("list", 0, [1])), {117: 4}, {0: L + '[{"insert":[1]}]'})
    add("an insert interrupted by an anchor", 118, lambda r: (r.text_insert("text", 0, "ad"), r.commit(), r.text_insert("text", 1, "bc"), r.text_mark("text", 2, 3, "bold", True)),
        {118: 2}, {0: T + '[{"retain":1},{"insert":"bc"}]'})
    add("list values of every plain kind", 119, lambda r: r.list_insert("list", 0, [None, True, False, 0, -1, 1.5, -0.0, "s\"\n", b"\x00\xff", [1, [2]], {"b": 1, "a": {"c": []}}]), {},
        {0: L + '[{"insert":[null,true,false,0,-1,1.5,-0.0,"s\\"\\n",[0,255],[1,[2]],{"a":{"c":[]},"b":1}]}]'})
    add("list retain, insert, delete", 120, lambda r: (r.list_insert("list", 0, [1, 2, 3, 4]), r.commit(), r.list_delete("list", 1, 2), r.list_insert("list", 1, ["x"])),
        {120: 4}, {0: L + '[{"retain":1},{"insert":["x"]},{"delete":2}]'})
    add("a list counts elements in both units", 121, lambda r: (r.list_insert("list", 0, [ASTRAL, 2]), r.commit(), r.list_delete("list", 1, 1)), {121: 2},
        {0: L + '[{"retain":1},{"delete":1}]', 1: L + '[{"retain":1},{"delete":1}]'})
    add("map write only", 122, lambda r: (r.text_insert("text", 0, "a"), r.commit(), r.map_set("m", "k", 1)), {122: 1}, {0: ""}, 1)
    add("map write below A only", 123, lambda r: (r.map_set("m", "k", 1), r.commit(), r.text_insert("text", 0, "a")), {123: 1}, {0: T + '[{"insert":"a"}]'}, 0)
    add("A cuts inside a MovableList insert row", 124, lambda r: r.mlist_insert("ml", 0, [1, 2, 3]), {124: 2}, {0: ""}, 1)
    add("A at the end of a MovableList insert row", 125, lambda r: (r.mlist_insert("ml", 0, [1, 2, 3]), r.text_insert("text", 0, "a")), {125: 3}, {0: T + '[{"insert":"a"}]'}, 0)

    def kids(r):
        a = r.list_insert_container("list", 0, wire.KIND_LIST)           # (126, 0)
        r.list_insert(a, 0, [1]); r.commit()                             # (126, 1)
        b = r.list_insert_container(a, 1, wire.KIND_TEXT)                # (126, 2)
        r.text_insert(b, 0, "in"); r.list_delete(a, 0, 1)                # (126, 3..4), (126, 5)
        r.list_insert_container("list", 1, wire.KIND_MAP)                # (126, 6)
        r.list_insert_container("list", 2, wire.KIND_MOVABLE)            # (126, 7)
    add("children of a List, a grandchild, a Map and a MovableList child", 126, kids, {126: 2},
        {0: '"cid:0@126:List":[{"insert":["\U0001F99C:cid:2@126:Text"]},{"delete":1}],"cid:2@126:Text":[{"insert":"in"}],'
            + L + '[{"retain":1},{"insert":["\U0001F99C:cid:6@126:Map","\U0001F99C:cid:7@126:MovableList"]}]'}, 0)
    add("member order: cid:10@ sorts in front of cid:2@", 127,
        lambda r: [r.text_insert(r.map_set_container("m", "k%d" % k, wire.KIND_TEXT), 0, "%x" % k) for k in range(6)], {},
        {0: '"cid:0@127:Text":[{"insert":"0"}],"cid:10@127:Text":[{"insert":"5"}],"cid:2@127:Text":[{"insert":"1"}],"cid:4@127:Text":[{"insert":"2"}],'
            '"cid:6@127:Text":[{"insert":"3"}],"cid:8@127:Text":[{"insert":"4"}]'}, 1)
    add("root names: a prefix, an escape, a multi-byte name", 128,
        lambda r: [r.text_insert(n, 0, "x") for n in ("ab", "a", "a\"b", "é", "a-")], {},
        {0: '"cid:root-a-:Text":[{"insert":"x"}],"cid:root-a:Text":[{"insert":"x"}],"cid:root-a\\"b:Text":[{"insert":"x"}],"cid:root-ab:Text":[{"insert":"x"}],'     # - : \\ b
            '"cid:root-é:Text":[{"insert":"x"}]'})
    add("V is a checkout: what lies beyond it is not there", 129, lambda r: (r.text_insert("text", 0, "ab"), r.commit(), r.text_insert("text", 2, "cd"), r.commit(), r.text_delete("text", 0, 1)),
        {129: 2}, {0: T + '[{"retain":2},{"insert":"c"}]'}, 0, [(129, 2)])
    add("V is a checkout inside a delete row", 130, lambda r: (r.text_insert("text", 0, "abcdef"), r.commit(), r.text_delete("text", 1, 4)),
        {130: 6}, {0: T + '[{"retain":1},{"delete":3}]'}, 0, [(130, 8)])

    def two(r):
        r.text_insert("text", 0, "abc"); r.commit()
        o = wire.Replica(132); o.merge_from(r); o.set_visible("text", wire.KIND_TEXT, list(r.seq[wire.root_cid("text", wire.KIND_TEXT)]))
        o.text_delete("text", 1, 1); o.commit()                          # both delete b, concurrently
        r.text_delete("text", 1, 1); r.commit()
        return o
    r = wire.Replica(131); o = two(r)
    d = Doc("two deleters", [r, o])
    for name, a, e in (("one of two deleters in A", {131: 4}, ""), ("neither deleter in A", {131: 3}, '"cid:root-text:Text":[{"retain":1},{"delete":1}]'),
                       ("the other peer's deleter in A (an open vector)", {131: 3, 132: 1}, "")):
        out.append((name, d, a, None, {0: ("{" + e + "}").encode()}, 0))
    add("A beyond V", 133, lambda r: r.text_insert("text", 0, "a"), {133: 2}, {0: None})
    return out


# ------------------------------------------------------------------------------------- documents built on the kernels' boundaries
def _mixed(n, seed):
    """n scalars mixing the escapes and every UTF-8 length, so that the lanes' stores straddle"""
    rng = random.Random(seed)
    return "".join(rng.choice(['"', "\\", "\n", "\x01", "a", "é", "中", ASTRAL, "z"]) for _ in range(n))


def _classes_of(d, fr_a, key="text", kind=wire.KIND_TEXT, fr_v=None):
    m = d.model
    return "".join(k for k, _ in classes(m, wire.root_cid(key, kind), m.version(fr_a), m.version(fr_v)))


def chunk_docs():
    """class changes at element index 62 … 65 and 126 … 129 of one Text and one List of L elements: the first version holds L elements;
    then, at index s, (K→I) an insert of 3, (K→D) a delete of 3, (I→D→K) an insert of 2 in front of a delete of 2.  The builder
    asserts the class string from the model.  -> [(Doc, [frontiers of A])]"""
    out = []
    for L in (63, 64, 65, 127, 128, 129, 130, 200):
        for s in (62, 63, 64, 65, 126, 127, 128, 129):
            if s + 4 > L and s != L:
                continue
            for how in ("KI", "KD", "IDK"):
                if s == L and how != "KI":
                    continue

                def build(r):
                    r.text_insert("text", 0, "".join("abcdefghij"[k % 10] for k in range(L)))
                    r.list_insert("list", 0, list(range(L)))
                    r.commit()
                    if how != "KI":
                        r.text_delete("text", s, 3 if how == "KD" else 2); r.list_delete("list", s, 3 if how == "KD" else 2)
                    if how != "KD":
                        r.text_insert("text", s, "XYZ"[:3 if how == "KI" else 2]); r.list_insert("list", s, ["X", "Y", "Z"][:3 if how == "KI" else 2])
                d, _ = _doc("L=%d %s at %d" % (L, how, s), 70, build)
                a = [(70, 2 * L - 1)]
                want = "K" * s + {"KI": "III", "KD": "DDD", "IDK": "IIDD"}[how] + "K" * (L - s - {"KI": 0, "KD": 3, "IDK": 2}[how])
                assert _classes_of(d, a) == want and _classes_of(d, a, "list", wire.KIND_LIST) == want, d.label
                out.append((d, [a]))
    return out


def gap_docs():
    """insert gaps of 63 / 64 / 65 / 200 mixed scalars behind 0, 1 and 62 retained ones (one insert op that goes on across the chunk
    edge), the same as a List of strings (first_item places the comma); a gap interrupted by a D, by an anchor and by an element that
    is in neither version"""
    out = []
    for n in (63, 64, 65, 200):
        for lead in (0, 1, 62):
            def build(r):
                r.text_insert("text", 0, "k" * lead + "TAIL"); r.list_insert("list", 0, [0] * lead + ["tail"]); r.commit()
                r.text_insert("text", lead, _mixed(n, n + lead)); r.list_insert("list", lead, [c * 2 for c in _mixed(n, n)])
            d, _ = _doc("gap of %d behind %d" % (n, lead), 71, build)
            a = [(71, 2 * lead + 4)]
            assert _classes_of(d, a) == "K" * lead + "I" * n + "KKKK", d.label
            out.append((d, [a]))

    def interrupted(r):
        r.text_insert("text", 0, "a" + "d" * 70 + "z"); r.commit()                           # ctr 0..71
        r.text_insert("text", 1, "I" * 40)                                                   # a I*40 d*70 z
        r.text_insert("text", 43, "J" * 30)                                                  # a I*40 d d J*30 d*68 z
        r.text_delete("text", 41, 2)                                                         # the two d's between the inserts
        r.text_mark("text", 45, 55, "bold", True)                                            # anchors inside the J's
        r.text_insert("text", 20, "gone"); r.text_delete("text", 20, 4)                      # in neither version, inside the I's
        r.text_delete("text", 93, 40)                                                        # (73 entities in front of the d's)
    d, _ = _doc("an interrupted gap", 72, interrupted)
    assert _classes_of(d, [(72, 71)]) == "K" + "I" * 40 + "DD" + "I" * 30 + "K" * 20 + "D" * 40 + "K" * 9, _classes_of(d, [(72, 71)])
    out.append((d, [[(72, 71)]]))
    return out


def astral_docs():
    """an astral scalar at index 63 / 64 / 65 as K, as D, and as the last scalar of a retain"""
    out = []
    for at in (63, 64, 65):
        for how in ("K", "D", "last"):
            def build(r):
                r.text_insert("text", 0, "x" * at + ASTRAL + "y" * 5); r.commit()
                if how == "D":
                    r.text_delete("text", at, 1)
                elif how == "last":
                    r.text_insert("text", at + 1, "!")
                else:
                    r.text_delete("text", at + 2, 1)
            d, _ = _doc("astral %s at %d" % (how, at), 73, build)
            a = [(73, at + 5)]
            cl = classes(d.model, wire.root_cid("text", wire.KIND_TEXT), d.model.version(a), d.model.all_ids)
            assert cl[at][0] == ("D" if how == "D" else "K") and ord(cl[at][1].what[1]) >= 0x10000, d.label
            out.append((d, [a]))
    return out


def delete_row_docs():
    """forward and backward delete runs of 5 (one delete op each): A at each of the six cuts, V (a checkout) at each of the six cuts;
    a delete of another peer's elements; single-peer documents (element slot = counter) deleting the slots [30, 34), [31, 33), [0, 32),
    [32, 64), [63, 66) and a run of 100, forward and backward.  -> [(Doc with its V's as versions, [frontiers of A])]"""
    out = []
    for back in (False, True):
        def build(r):
            r.text_insert("text", 0, "abcdefghij"); r.commit()                               # ctr 0..9
            for k in range(5):
                r.text_delete("text", 6 - k if back else 2, 1)                              # ctr 10..14: one op
        r = wire.Replica(74); build(r); r.commit()
        ops = [op for c in r.changes[74] for op in c.ops if op.kind == "delete"]
        assert len(ops) == 1 and ops[0].signed_len == (-5 if back else 5)
        cuts = [[(74, 9 + k)] for k in range(6)]
        d = Doc("%s run of 5" % ("backward" if back else "forward"), [r], [("cut %d" % k, c) for k, c in enumerate(cuts)])
        for k, c in enumerate(cuts):               # the k atoms in front of the cut are in the version: forward hits c d e f g in order
            gone = sum(1 for x, _ in classes(d.model, wire.root_cid("text", wire.KIND_TEXT), d.model.version([(74, 9)]), d.model.version(c)) if x == "D")
            assert gone == k, d.label
        out.append((d, cuts))
    a, b = wire.Replica(75), wire.Replica(76)
    a.text_insert("text", 0, "0123456789" * 7); a.commit()
    b.merge_from(a); b.set_visible("text", wire.KIND_TEXT, list(a.seq[wire.root_cid("text", wire.KIND_TEXT)]))
    b.text_delete("text", 60, 8); b.text_insert("text", 60, "B"); b.commit()
    out.append((Doc("another peer's elements", [a, b], [("b only half", [(76, 3)])]), [[(75, 69)], [(75, 69), (76, 3)], [(75, 30)]]))
    for lo, hi in ((30, 34), (31, 33), (0, 32), (32, 64), (63, 66), (20, 120)):
        for back in (False, True):
            def build(r):
                r.text_insert("text", 0, "".join(chr(97 + k % 26) for k in range(130))); r.commit()     # slot = counter 0..129
                for k in range(hi - lo):
                    r.text_delete("text", hi - 1 - k if back else lo, 1)
            d, _ = _doc("slots [%d, %d) %s" % (lo, hi, "backward" if back else "forward"), 77, build)
            ops = [op for c in d.reps[0].changes[77] for op in c.ops if op.kind == "delete"]
            assert len(ops) == 1 and ops[0].del_id == (77, lo) and abs(ops[0].signed_len) == hi - lo, d.label
            mid = [(77, 129 + (hi - lo) // 2)]
            d.versions.append(("half of the run", mid))
            out.append((d, [[(77, 129)], mid, [(77, 130)]]))
    return out


def many_peer_docs():
    """documents of 1 / 2 / 63 / 64 / 65 / 255 peers; every peer writes three scalars into the Text (one survives, one is deleted by
    its own peer later, one is inserted later); A names a subset of the peers (every third one left out, every fifth one behind its
    delete) and stands at counter 2 of the peers with index 63 / 64 / 65 / 254, so that their elements occur as K, I, D and skipped —
    every class, which the builder asserts per index"""
    out = []
    for n in (1, 2, 63, 64, 65, 255):
        reps, a = [], {}
        for k in range(n):
            r = wire.Replica(2000 + 7 * k if k < n - 5 or n < 6 else EDGE_PEERS[k - (n - 5)])
            r.text_insert("text", 0, "%c%c" % (97 + k % 26, 65 + k % 26)); r.commit()         # ctr 0, 1
            r.text_delete("text", 1, 1); r.text_insert("text", 1, ASTRAL if k % 4 == 0 else "+"); r.commit()     # ctr 2, 3
            r.text_insert("text", 0, "t"); r.text_delete("text", 0, 1); r.commit()            # ctr 4, 5: in neither version
            reps.append(r)
            a[r.peer] = 2 if k in (63, 64, 65, 254) else 0 if k % 3 == 1 else 3 if k % 5 == 2 else 2
        d = Doc("%d peers" % n, reps)
        A, per = vector_ids(a), {}
        order = sorted(r.peer for r in reps)          # the stored peer index is the rank of the peer id
        assert order == [r.peer for r in reps]
        T = wire.root_cid("text", wire.KIND_TEXT)
        shown = {e.id: c for c, e in classes(d.model, T, A, d.model.all_ids)}
        for e in d.model.seqs[T]:
            per.setdefault(order.index(e.id[0]), set()).add(shown.get(e.id, "S"))      # S: in neither version, skipped
        for idx in (63, 64, 65, 254):
            if idx < n:
                assert per[idx] == set("KIDS"), (d.label, idx, per[idx])
        if n >= 3:
            assert per[1] == set("IS") and per[2] == set("KIS"), d.label             # a peer A does not name; a peer half way
        out.append((d, a))
    return out


def edge_peer_child_docs():
    """children created by each of EDGE_PEERS, inserted into one List: the payload string and the child's own key carry the peer id"""
    reps = []
    for k, p in enumerate(EDGE_PEERS):
        r = wire.Replica(p)
        c = r.list_insert_container("list", 0, wire.KIND_TEXT if k % 2 else wire.KIND_LIST)
        if k % 2:
            r.text_insert(c, 0, "p%d" % k)
        else:
            r.list_insert(c, 0, [k])
        r.commit()
        reps.append(r)
    return Doc("children of the edge peers", reps)


def member_docs():
    """63 / 64 / 65 / 130 child Texts with a non-empty delta each (their counters have one, two and three digits: key order is not table
    order), and the root names of _cursor_ref.container_docs with one that needs escaping"""
    out = []
    for d in _cursor_ref.container_docs():
        out.append(d)

    def names(r):
        for k, name in enumerate(["q\"uote", "back\\slash", "tab\tname", "a", "a\x01"]):
            r.text_insert(name, 0, "v%d" % k); r.list_insert(name + "~", 0, [k])
    out.append(_doc("names that need escaping", 78, names)[0])
    return out


def payload_doc():
    """one List insert holding a thinned f64 / i64 corpus, strings with every escape, bytes, nested lists and dicts with keys"""
    import _values
    vals = [_values.f64_of(b) for b in _values.f64_subset()[::40]] + _values.i64_corpus()[::3] + _values.str_corpus()[::7]
    vals += [b"", b"\x00", bytes(range(256)), [], [[]], [1, [2.5, ["x", {"k": None}]]], {}, {"": 0}, {"k\"": [1, {"é": b"\x01"}], "a": {"b": {"c": True}}}]
    return _doc("payloads", 79, lambda r: (r.list_insert("list", 0, [0]), r.commit(), r.list_insert("list", 1, vals)))[0], [(79, 0)]


def call_queries(d, n):
    """n different A's on one single-writer document: every counter as a frontier, cyclically"""
    end = max(c for _, c in d.model.all_ids) + 1
    return [[(d.reps[0].peer, (7 * k) % end)] for k in range(n)]


def boundary_entries():
    """every hand-built document with its A's -> [Entry]"""
    out = []

    def add(d, a_list, v_list=(None,)):
        for fr in v_list:
            e = Entry(d, "latest" if fr is None else "checkout %r" % (fr,), fr)
            e.ask("empty", frozenset(), None)
            for a in a_list:
                e.ask(repr(a)[:60], vector_ids(a) if isinstance(a, dict) else d.model.version(a))
            out.append(e)
    for d, a in chunk_docs() + gap_docs() + astral_docs():
        add(d, a)
    for d, a in delete_row_docs():
        add(d, a, [fr for _, fr in d.versions])
    for d, a in many_peer_docs():
        add(d, [a])
    add(edge_peer_child_docs(), [])
    for d in member_docs():
        add(d, [[(d.reps[0].peer, max(c for p, c in d.model.all_ids if p == d.reps[0].peer) // 2)]])
    d, a = payload_doc()
    add(d, [a])
    for d in _cursor_ref.leaf_docs():
        add(d, call_queries(d, 9))
    for name, d, a, v, _, _ in literals():
        add(d, [a], [v])
    return out


def merge_docs_entries():
    """the linear-prefix documents, every eighth sweep document and the backspace documents of _merge_docs at each of their versions"""
    docs = _merge_docs.linear_prefix_docs() + _merge_docs.sweep_docs()[::8] + _merge_docs.backspace_docs()
    for d in docs:
        d.versions = [("latest", None)] + [("version %d" % k, fr) for k, fr in enumerate(d.versions)]
    return entries_of(docs)[0]


def run_state_snapshots(ctx, docs, what="state-staged snapshots"):
    """each document as ONE snapshot, staged from its state section (the first delta call stages it once more through its history);
    asked from every recorded version.  The state section's bytes are the oracle's state writer's, the expectation is the model's"""
    import _oracle
    snaps = []
    for d in docs:
        full = wire.Replica(d.reps[0].peer)
        for r in d.reps:
            full.merge_from(r)
        st, ents = _oracle.state_entries([full.export()])
        assert st == 0
        snaps.append([full.export_snapshot(state=ents)])
    res = ctx.merge_batch(snaps)
    assert ctx.b.state_documents(ctx.h) == len(docs) and [r[:2] for r in res] == [d.model.result()[:2] for d in docs], what
    n = 0
    for units in (0, 1):
        qs, exs = [], []
        for i, d in enumerate(docs):
            for _, fr in d.versions:
                A = d.model.version(fr) if fr is not None else frozenset()
                qs.append((i, wire.encode_vv(vector_of(A)) if A else None)); exs.append(Expect(d.model, A, d.model.all_ids, units))
        for g, ex in zip(ctx.delta(qs, units), exs):
            check_one(g, ex, what)
        n += len(qs)
    assert ctx.fetch() == res, what
    return n


def run_failed_step(ctx):
    """A resident document whose second step carries a damaged blob (its last byte flipped: the envelope checksum no longer fits,
    LM_CHECKSUM_MISMATCH = 2).  Literals, by the header ("the document's own import error for a failed document", loro_merge.h:458)
    and the driver (Engine::delta_bounds, lm_pipeline.h:2078 `if (m.status != ST_OK) { o.status = m.status; return false; }` — no
    launch, no bytes, other_changed 0): every query on the document answers the step's error until a step goes through, whatever
    its A — well-formed, beyond the document or no version vector at all.  The step delivered once more goes through, and the
    document answers from the version that survived (the vector after step 0), from inside it and from the empty version"""
    a = wire.Replica(7)
    a.text_insert("text", 0, "hello"); a.commit()                                         # (7, 0..4)
    first = a.export()
    a.text_insert("text", 5, "!"); a.text_delete("text", 0, 1); a.map_set("m", "k", 1); a.commit()      # (7, 5), (7, 6), (7, 7)
    second = a.export({7: 5})
    T = b'{"cid:root-text:Text":'
    ctx.stage([[first]]); ctx.run()
    stood = ctx.fetch()
    assert stood[0][:3] == (0, b'{"text":"hello"}', wire.encode_vv({7: 5}))
    assert ctx.delta([(0, None), (0, wire.encode_vv({7: 5}))]) == [(OK, 0, T + b'[{"insert":"hello"}]}'), (OK, 0, b"{}")]
    bad = bytearray(second); bad[-1] ^= 1
    res = ctx.step([[bytes(bad)]])
    assert res[0][0] == 2, res
    qs = [(0, None), (0, wire.encode_vv({7: 5})), (0, wire.encode_vv({7: 2})), (0, wire.encode_vv({7: 9})), (0, b"\xff")]
    assert ctx.delta(qs) == [(2, 0, b"")] * 5
    assert ctx.delta(qs, 1) == [(2, 0, b"")] * 5
    res = ctx.step([[second]])
    assert res[0][:3] == (0, b'{"m":{"k":1},"text":"ello!"}', wire.encode_vv({7: 8}))
    assert ctx.delta(qs + [(0, wire.encode_vv({7: 7})), (0, wire.encode_vv({7: 8}))]) == [
        (OK, 1, T + b'[{"insert":"ello!"}]}'), (OK, 1, T + b'[{"delete":1},{"retain":4},{"insert":"!"}]}'),
        (OK, 1, T + b'[{"delete":1},{"retain":1},{"insert":"llo!"}]}'), (FRONTIERS_NOT_FOUND, 0, b""), (1, 0, b""),
        (OK, 1, b"{}"), (OK, 0, b"{}")]
    assert ctx.fetch() == res


def run_zero_row_document(ctx):
    """a document without a blob — zero op rows, zero peers, status 0 — between two queried documents: its query owns no workgroup of
    k_delta_mark, so two neighbouring queries have the same `row_blk0` and dl_mark_row's search must give every workgroup to the
    LAST of them (lm_k_delta.h:74); asked twice in a row, and in front of and behind documents that have rows"""
    r = wire.Replica(81); r.text_insert("text", 0, "abc"); r.commit(); r.text_delete("text", 1, 1); r.commit()
    s = wire.Replica(82); s.list_insert("list", 0, [1, 2, 3]); s.commit(); s.list_delete("list", 0, 2); s.commit()
    d1, d2 = Doc("rows in front", [r]), Doc("rows behind", [s])
    res = ctx.merge_batch([d1.blobs, [], d2.blobs, []])
    assert res == [d1.model.result(), (0, b"{}", wire.encode_vv({}), 0), d2.model.result(), (0, b"{}", wire.encode_vv({}), 0)]
    a1, a2 = wire.encode_vv({81: 3}), wire.encode_vv({82: 3})
    w1 = (OK, 0, b'{"cid:root-text:Text":[{"retain":1},{"delete":1}]}')
    w2 = (OK, 0, b'{"cid:root-list:List":[{"delete":2}]}')
    e = (OK, 0, b"{}")
    assert ctx.delta([(0, a1), (1, None), (2, a2)]) == [w1, e, w2]
    assert ctx.delta([(1, None), (1, None), (0, a1), (3, None), (1, wire.encode_vv({})), (2, a2), (3, None)]) == [e, e, w1, e, e, w2, e]
    assert ctx.delta([(1, wire.encode_vv({81: 1}))]) == [(FRONTIERS_NOT_FOUND, 0, b"")]
    assert ctx.fetch() == res
