"""Stable cursors (lm_cursor_pos / lm_cursor_at) restated over the PLAIN merge model (tests/_merge_ref.py): the expected answers, the
corpora and the documents built on k_cursor's boundaries, shared by test_cursor_ref.py (kernel-logic harness) and
test_gpu_zz_cursor_ref.py (device).  The expectation is the model alone: no call into the oracle, no oracle JSON (the query lists and
the comparison are _cursor.py's, which this module imports).

The rules.  For a sequence container `cid` of a Model (or of a Session's model after a step) at a version V (a set of ids; frontiers
None = everything applied):
  order     = Model.sequence_ids(cid): every element ever inserted, in sequence order;
  entities  = the ids of `order` visible at V (Model.visible_ids(cid, frontiers)); an entity is a scalar or a style anchor;
  scalars   = the entities that are not anchors (`what[0]` of the element is "start" / "end" for an anchor); a List has scalars only;
  a scalar is 2 UTF-16 units wide from U+10000 on, else 1.
lm_cursor_pos(id, side)
  * no id: (OK, 0 for Left else the length in scalars, the same in UTF-16 units, side)       state.rs:2073-2090 (Left: :2074-2076)
  * id visible at V: OK, pos = the scalars in front of it among the entities, side unchanged.  state.rs:2064-2067 get_text_index_of_id
    with the event index: the entity index converted as handler.rs:2737-2745 converts it — anchors are not counted, so an anchor answers
    with the position of the next scalar.
  * id in V, not visible at V: (DELETED, the scalars among the entities in front of it in `order`, …, Left).  loro.rs:1883-1948: the
    reference replays the container to where the id was deleted, takes get_id_latest_pos — the visible entities in front of the
    tombstone — and converts it with convert_entity_index_to_event_index (:1937-1940); the side comes from the tracker (Left).
  * anything else — an id outside V, an id delivered but pending, an id of another container (a delete's own op id among them), a
    peer the document does not hold, a counter < 0 or >= 2^24: (ID_NOT_FOUND, 0, 0, side).  loro.rs:1911-1917: no delete op names it.
lm_cursor_at(pos, side)                                                                        handler.rs:2673-2745
  * an empty container: (OK, no id, Left for Middle else side, 0)                              :2704-2715
  * pos >= length: (OK, no id, Right, length)                                                  :2717-2724
  * else (OK, the id of scalar `pos`, side, pos): the position is an event index, an anchor is never returned   :2726-2733
This reproduces every literal of _cursor.hand_cases() (test_cursor_ref.py::test_the_restatement_gives_the_hand_written_answers runs
first); nothing that _cursor.Expect pins had to change.

A child whose creating entry is not visible (an overwritten Map key, a deleted List element).  has_container (loro.rs:1135-1142 →
state.rs:968-984) is true for every container the arena has a depth for, whether reachable from a root or not, and a container's
state is made when its first op is applied (diff_calc.rs:299), not when its parent shows it: get_relative_position (state.rs:2061-2091)
answers from that state.  So the rules above hold for such a child unchanged, at the latest version and at any version in which it has
an element; at a version in which it has none, every id is outside V and a query without an id answers 0 either way (a state that
holds nothing, or loro.rs:1980-1996: the handler's length).  `unreachable_child_case` pins it as literals, `empty_container_case`
pins a container in front of its first op.

Corpora: see the docstring of test_cursor_ref.py for the floors and the counts."""
import random

import _cursor, _fuzz, _merge_ref
from _cursor import OK, DELETED, NOT_FOUND, NO_CONTAINER, UNSUPPORTED, LEFT, MIDDLE, RIGHT
from _richtext_ref import changes_of
from loro_amd import wire

KIND_NAME = {wire.KIND_TEXT: "Text", wire.KIND_LIST: "List", wire.KIND_MAP: "Map", wire.KIND_MOVABLE: "MovableList"}
SIDES = (LEFT, MIDDLE, RIGHT)


def cid_str(cid):
    """ContainerID Display"""
    if cid.root:
        return "cid:root-%s:%s" % (cid.name, KIND_NAME[cid.kind])
    return "cid:%d@%d:%s" % (cid.counter, cid.peer, KIND_NAME[cid.kind])


def sequence_cids(model):
    """the Text / List containers of a model that hold an element"""
    return [c for c in model.sequences() if c.kind in (wire.KIND_TEXT, wire.KIND_LIST)]


class Expect:
    """one sequence container of a model at one version"""

    def __init__(self, model, cid, frontiers=None):
        self.cid, self.key = cid, cid_str(cid)
        V = self.V = model.version(frontiers)
        self.order = model.sequence_ids(cid)
        self.entities = model.visible_ids(cid, frontiers)
        what = {e.id: e.what for e in model.seqs.get(cid, ())}
        self.anchors = {i for i, w in what.items() if w[0] in ("start", "end")}
        assert cid.kind == wire.KIND_TEXT or not self.anchors
        self.vis = set(self.entities)
        self.scalars = [i for i in self.entities if i not in self.anchors]
        self.length = len(self.scalars)
        self.wide = {i for i, w in what.items() if w[0] == "char" and ord(w[1]) >= 0x10000}
        self.vv = {}
        for p, c in V:
            self.vv[p] = max(self.vv.get(p, 0), c + 1)
        # per index of `order`: entities / scalars / UTF-16 units visible in front of it
        self.index = {i: k for k, i in enumerate(self.order)}
        self.ent_before, self.sc_before, self.u16_before = [], [], []
        ne = ns = nu = 0
        for i in self.order:
            self.ent_before.append(ne); self.sc_before.append(ns); self.u16_before.append(nu)
            if i in self.vis:
                ne += 1
                if i not in self.anchors:
                    ns += 1; nu += 2 if i in self.wide else 1
        self.length16 = nu

    def pos_answer(self, id_, side):
        """(status, pos, pos_utf16, side) of lm_cursor_pos"""
        if id_ is None:
            return (OK, 0, 0, side) if side == LEFT else (OK, self.length, self.length16, side)
        k = self.index.get(tuple(id_))
        if k is not None and id_ in self.vis:
            return (OK, self.sc_before[k], self.u16_before[k], side)
        if k is not None and id_ in self.V:
            return (DELETED, self.sc_before[k], self.u16_before[k], LEFT)
        return (NOT_FOUND, 0, 0, side)

    def at_answer(self, pos, side):
        """(status, id, side, origin_pos) of lm_cursor_at"""
        if self.length == 0:
            return (OK, None, LEFT if side == MIDDLE else side, 0)
        if pos >= self.length:
            return (OK, None, RIGHT, self.length)
        return (OK, self.scalars[pos], side, pos)


def queries(doc, ex, other_ids=(), positions=True):
    """every id of `order`, the extras of _cursor.container_queries, every position -> (pq, pw, aq, aw)"""
    (pq, pw), (aq, aw) = _cursor.container_queries(doc, ex.key, ex, None, other_ids)
    if not positions:
        aq, aw = aq[-3:], aw[-3:]
    return pq, pw, aq, aw


def document_queries(doc, model, frontiers=None, positions=True):
    """the queries of every sequence container of a document, in one list -> (pq, pw, aq, aw, [Expect])"""
    exs = [Expect(model, c, frontiers) for c in sequence_cids(model)]
    pq, pw, aq, aw = [], [], [], []
    for k, ex in enumerate(exs):
        other = exs[(k + 1) % len(exs)].order if len(exs) > 1 else ()
        a, b, c, d = queries(doc, ex, other, positions)
        pq += a; pw += b; aq += c; aw += d
    return pq, pw, aq, aw, exs


# ------------------------------------------------------------------------------------------------- counts, from the model alone
COUNTS = ("pos_not_entity_index", "cursor_is_anchor", "deleted_behind_anchor", "pos16_differs", "over_64_entities", "over_64_runs",
          "deleted", "not_found", "ok")


def runs_of(ex):
    """a lower bound of the container's items: maximal stretches of `order` with consecutive ids and one visibility"""
    n, prev = 0, None
    for i in ex.order:
        cur = (i[0], i[1], i in ex.vis)
        if prev is None or (prev[0], prev[1] + 1, prev[2]) != cur:
            n += 1
        prev = cur
    return n


def count(exs, pqs, pws):
    """COUNTS over containers `exs` and their lm_cursor_pos queries / answers"""
    tot = dict.fromkeys(COUNTS, 0)
    by_key = {}
    for ex in exs:
        by_key.setdefault((ex.doc, ex.key), ex)
        tot["over_64_entities"] += len(ex.entities) > 64
        tot["over_64_runs"] += runs_of(ex) > 64
    for q, w in zip(pqs, pws):
        ex = by_key[(q[0], q[1])]
        tot["ok"] += w[0] == OK; tot["deleted"] += w[0] == DELETED; tot["not_found"] += w[0] == NOT_FOUND
        if q[2] is None or w[0] not in (OK, DELETED):
            continue
        k = ex.index[tuple(q[2])]
        tot["pos_not_entity_index"] += w[1] != ex.ent_before[k]
        tot["cursor_is_anchor"] += w[0] == OK and q[2] in ex.anchors
        tot["deleted_behind_anchor"] += w[0] == DELETED and w[1] != ex.ent_before[k]
        tot["pos16_differs"] += w[2] != w[1]
    return tot


# ------------------------------------------------------------------------------------------------------------------- the documents
class Doc:
    """a document (its blobs, the writers' changes and their model) and the versions it is asked at: [(label, frontiers or None)]"""

    def __init__(self, label, reps, versions=(), blobs=None):
        self.label, self.reps = label, reps
        self.changes = changes_of(reps)
        self.model = _merge_ref.Model(self.changes)
        self.blobs = blobs if blobs is not None else _fuzz.blobs_of(reps)
        self.versions = [("latest", None)] + [(l, list(f)) for l, f in versions]


def _version_set(reps, snaps, rng):
    """every recorded frontier (multi-head ones among them), a change end, a version inside a change, a frontier of two concurrent peers"""
    out, seen = [], set()

    def add(label, fr):
        key = tuple(sorted(fr))
        if key and key not in seen:
            seen.add(key); out.append((label, list(fr)))
    for k, (fr, _) in enumerate(snaps):
        add("snapshot %d" % k, fr)
    own = [(r, r.changes.get(r.peer, [])) for r in reps if r.changes.get(r.peer)]
    r, chs = rng.choice(own)
    ch = rng.choice(chs)
    add("change end", [(ch.peer, ch.ctr_end - 1)])
    long_ = [c for _, cs in own for c in cs if c.ctr_end - c.counter >= 3]
    if long_:
        ch = rng.choice(long_)
        add("inside a change", [(ch.peer, rng.randrange(ch.counter, ch.ctr_end - 1))])
    if len(own) >= 2:
        m = _merge_ref.Model(changes_of(reps))
        for _ in range(40):
            (ra, ca), (rb, cb) = rng.sample(own, 2)
            a, b = rng.choice(ca), rng.choice(cb)
            fa, fb = (a.peer, a.ctr_end - 1), (b.peer, b.ctr_end - 1)
            if fa not in m.closure_of_id(fb) and fb not in m.closure_of_id(fa):
                add("two concurrent peers", [fa, fb])
                break
    return out


def rich_docs(seeds):
    """styled Text (and List) sessions of three peers whose writers took their views from the model"""
    docs = []
    for seed in seeds:
        snaps = []
        kinds = ("text",) if seed % 2 == 0 else ("text", "list")
        reps = _fuzz.random_session(seed, n_peers=3, n_steps=130 if seed % 2 == 0 else 160, kinds=kinds, styles="rich", view=_merge_ref.view, snapshots=snaps,
                                    max_ins=[6, 12][seed % 3 == 0])
        docs.append(Doc("rich %d" % seed, reps, _version_set(reps, snaps, random.Random(seed))))
    return docs


def nested_docs(seeds):
    """child Text / List inside Map and List (every sequence container of the document is asked in one call)"""
    docs = []
    for seed in seeds:
        reps = _fuzz.nested_session(seed, n_peers=3, n_steps=160, view=_merge_ref.view)
        snaps = [([(r.peer, ch.ctr_end - 1)], None) for r in reps for ch in r.changes.get(r.peer, [])[2::5]]
        docs.append(Doc("nested %d" % seed, reps, _version_set(reps, snaps, random.Random(seed))))
    return docs


def small_version_docs():
    """a smaller corpus whose versions run IN FULL, three ways, under every setting: four styled and four nested sessions"""
    docs = []
    for seed in range(980, 984):
        snaps = []
        reps = _fuzz.random_session(seed, n_peers=3, n_steps=70, kinds=("text", "list"), styles="rich", view=_merge_ref.view, snapshots=snaps)
        docs.append(Doc("small rich %d" % seed, reps, _version_set(reps, snaps, random.Random(seed))))
    for seed in range(990, 994):
        reps = _fuzz.nested_session(seed, n_peers=3, n_steps=80, view=_merge_ref.view)
        snaps = [([(r.peer, ch.ctr_end - 1)], None) for r in reps for ch in r.changes.get(r.peer, [])[1::3]]
        docs.append(Doc("small nested %d" % seed, reps, _version_set(reps, snaps, random.Random(seed))))
    return docs


RICH_SEEDS, NESTED_SEEDS = range(900, 924), range(950, 974)
RICH_FLOORS = {"pos_not_entity_index": 200, "cursor_is_anchor": 50, "deleted_behind_anchor": 50, "pos16_differs": 50, "over_64_entities": 20, "over_64_runs": 20}
NESTED_FLOORS = {"deleted_in_children": 50}
VERSION_FLOORS = {"not_found_among_concurrent": 200, "visible_then_deleted": 100, "deleted_at_version": 100}


def entries(docs, versions="latest", positions=True):
    """the batch entries of `docs` -> (blobs per entry, frontiers per entry, pq, pw, aq, aw, [Expect], the model's result per entry)
    versions: "latest" (one entry per document), "all" (one per version)"""
    blobs, fronts, pq, pw, aq, aw, exs, want = [], [], [], [], [], [], [], []
    for d in docs:
        for label, fr in (d.versions if versions == "all" else d.versions[:1]):
            k = len(blobs)
            blobs.append(d.blobs); fronts.append(None if fr is None else wire.encode_frontiers(fr)); want.append(d.model.result(fr))
            a, b, c, e, xs = document_queries(k, d.model, fr, positions)
            for x in xs:
                x.doc, x.label = k, "%s at %s" % (d.label, label)
            pq += a; pw += b; aq += c; aw += e; exs += xs
    return blobs, fronts, pq, pw, aq, aw, exs, want


def version_counts(docs):
    """VERSION_FLOORS over the checked-out versions of `docs`"""
    tot = dict.fromkeys(VERSION_FLOORS, 0)
    for d in docs:
        latest = {c: Expect(d.model, c) for c in sequence_cids(d.model)}
        for label, fr in d.versions[1:]:
            for c, lx in latest.items():
                ex = Expect(d.model, c, fr)
                for k, i in enumerate(ex.order):
                    if i not in ex.V:
                        # an element of another peer that V holds stands on either side of it
                        before = any(j in ex.V and j[0] != i[0] for j in ex.order[max(0, k - 8):k])
                        after = any(j in ex.V and j[0] != i[0] for j in ex.order[k + 1:k + 9])
                        tot["not_found_among_concurrent"] += before and after
                    elif i in ex.vis:
                        tot["visible_then_deleted"] += i not in lx.vis
                    else:
                        tot["deleted_at_version"] += 1
    return tot


def check_floors(name, tot, floors):
    for k, least in floors.items():
        assert tot[k] >= least, (name, k, tot)


check = _cursor.check       # every query, status included, then the round trip


# ------------------------------------------------------------------------- the hand-written answers, for the restatement's own test
def hand_models():
    """[(name, Model of the case's writers, pos queries, expected, at queries, expected)] of _cursor.hand_cases().  The cases hand
    out blobs only; the replicas they are written with are recorded while the cases are built, and a case's writers are the recorded
    replicas whose export IS one of the case's blobs (however many a case uses or builds without exporting)"""
    made = []
    plain = wire.Replica

    class Recorded(plain):
        def __init__(self, peer):
            plain.__init__(self, peer)
            made.append(self)
    wire.Replica = Recorded
    try:
        cases = _cursor.hand_cases()
    finally:
        wire.Replica = plain
    exports = [(r.export(), r) for r in made if not r.pending_ops and r.changes]
    out = []
    for name, blobs, pq, pw, aq, aw in cases:
        writers = []
        for b in blobs:
            hit = [r for e, r in exports if e == b]
            assert hit, (name, "a blob that no recorded replica exports")
            writers.append(hit[0])
        out.append((name, _merge_ref.Model(changes_of(writers)), pq, pw, aq, aw))
    return out


def model_answers(model, pq, aq):
    """the answers of the rules above to queries by container KEY (a key that names no sequence container of the model: as the ABI
    says — UNSUPPORTED for a Map / MovableList the history holds, CONTAINER_NOT_FOUND otherwise)"""
    keys = {cid_str(c): c for c in list(model.seqs) + list(model.maps)}
    exs = {}

    def ex_of(key):
        c = keys.get(key)
        if c is None:
            return NO_CONTAINER
        if c.kind not in (wire.KIND_TEXT, wire.KIND_LIST):
            return UNSUPPORTED
        if key not in exs:
            exs[key] = Expect(model, c)
        return exs[key]
    pw, aw = [], []
    for _, key, id_, side in pq:
        ex = ex_of(key)
        pw.append((ex, 0, 0, side) if isinstance(ex, int) else ex.pos_answer(id_, side))
    for _, key, pos, side in aq:
        ex = ex_of(key)
        aw.append((ex, None, side, 0) if isinstance(ex, int) else ex.at_answer(pos, side))
    return pw, aw


# --------------------------------------------------------------------------------------- documents built on k_cursor's boundaries
ASTRAL = "\U0001F600"
EDGE_PEERS = [(1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]


def _one(label, peer, build):
    r = wire.Replica(peer)
    build(r)
    r.commit()
    return Doc(label, [r])


def window_docs():
    """step 2's windows (`e0 += 64`, `my_E < b_hi`): ONE insert of L scalars, then a mark whose StyleStart stands at entity 62 … 65 and
    whose End stands as far from the end; an astral scalar at entity 63 … 65; 70 StyleStarts in a row from entity 64 on (a window of
    anchors only); one tombstone whose entity index E is 63 … 65, 127 … 129 (E == b_hi = 64 / 128 with a window behind it where L
    allows) and one with nothing visible behind it (the conversion left pending when the walk ends).  The builder asserts from the
    model that the astral scalar and the tombstone stand at the entity index the label names"""
    docs = []
    for L in (63, 64, 65, 128, 129, 200):
        for s in (62, 63, 64, 65):
            if s + 1 < L - s:
                docs.append(_one("L=%d start at %d" % (L, s), 60, lambda r: (r.text_insert("text", 0, "x" * L), r.text_mark("text", s, L - s, "bold", True))))
            elif s < L:
                docs.append(_one("L=%d start at %d, to the end" % (L, s), 60, lambda r: (r.text_insert("text", 0, "x" * L), r.text_mark("text", s, L, "bold", True))))
        for a in (63, 64, 65):
            if a <= L:       # one StyleStart (entity 2) in front: scalar a - 1 is entity a
                d = _one("L=%d astral at entity %d" % (L, a), 61, lambda r: (r.text_insert("text", 0, "y" * (a - 1) + ASTRAL + "y" * (L - a)),
                                                                             r.text_mark("text", 2, min(a + 3, L), "link", "u")))
                ex = Expect(d.model, sequence_cids(d.model)[0])
                assert ex.entities[a] in ex.wide and len(ex.wide) == 1, d.label
                docs.append(d)
        # ASTRAL S z z E z …: L + 2 entities; the entity at index t is deleted, so the tombstone's entity index E is t
        for t in sorted({63, 64, 65, 127, 128, 129, L + 1}):
            if t < L + 2:
                d = _one("L=%d tombstone with E=%d%s" % (L, t, ", nothing behind it" if t == L + 1 else ""), 62,
                         lambda r: (r.text_insert("text", 0, ASTRAL + "z" * (L - 1)), r.text_mark("text", 1, 3, "bold", True), r.commit(), r.text_delete("text", t, 1)))
                ex = Expect(d.model, sequence_cids(d.model)[0])
                tomb = [i for i in ex.order if i not in ex.vis]
                assert len(tomb) == 1 and ex.ent_before[ex.index[tomb[0]]] == t and len(ex.entities) == L + 1, d.label
                docs.append(d)

    def anchors_only(r):
        r.text_insert("text", 0, "w" * 130)
        for _ in range(70):
            r.text_mark("text", 64, len(r.seq[wire.root_cid("text", wire.KIND_TEXT)]) - 1, "bold", True)
        r.commit()
        r.text_delete("text", 64 + 70, 1)           # the scalar behind the anchors: its tombstone converts behind a window of anchors
    docs.append(_one("70 anchors from entity 64", 63, anchors_only))
    return docs


def leaf_docs():
    """Texts of several leaves (every insert at the front is an item of its own): anchors and astral scalars in the first leaf, a
    stretch longer than a leaf in which nothing is visible with single tombstones around and inside it, a deleted tail, a container
    in which nothing is visible (a container that holds no element at all: `empty_container_case`)"""
    docs = []

    def many(r, n=230):
        for k in range(n):
            r.text_insert("text", 0, ("ab", ASTRAL + "c", "d")[k % 3])
        r.commit()
        T = wire.root_cid("text", wire.KIND_TEXT)
        for s in (1, 5, 9, 30):
            r.text_mark("text", s, s + 2, "bold", True)
        r.commit()
        return T

    def hole(r):
        T = many(r)
        r.text_delete("text", 80, 170)              # more than two leaves' worth of items without a visible element
        r.commit()
        r.text_delete("text", len(r.seq[T]) - 7, 7)  # the tail: nothing visible behind these tombstones
        r.text_delete("text", 3, 1); r.text_delete("text", 70, 2)
    docs.append(_one("three leaves", 64, many))
    docs.append(_one("a hole of leaves and a deleted tail", 65, hole))

    def nothing(r):
        many(r, 100)
        r.text_delete("text", 0, len(r.seq[wire.root_cid("text", wire.KIND_TEXT)]))
        r.list_insert("list", 0, [1, 2, 3]); r.commit(); r.list_delete("list", 0, 3)
    docs.append(_one("nothing visible", 66, nothing))
    return docs


def container_docs():
    """the container lookup (`c0 += 64`, the peer compare, bytes_eq): 63 / 64 / 65 / 130 child Texts of one Map; children with equal counters of
    different peers at the 2^32 / 2^63 edges; root names that are prefixes of each other, that differ in the last byte, a 300-byte
    name and a multi-byte one"""
    docs = []
    for n in (63, 64, 65, 130):
        def build(r):             # (children of one Map: a document holds at most 64 ROOT containers, lm_types.h MAX_ROOTS)
            kids = []
            for k in range(n):
                kids.append(r.map_set_container("m", "k%03d" % k, wire.KIND_TEXT))
                r.text_insert(kids[k], 0, "%c%d" % (97 + k % 26, k)); r.commit()
            for k in sorted({0, 62, min(63, n - 1), n - 1}):
                r.text_delete(kids[k], 0, 1)
        docs.append(_one("%d containers" % n, 67, build))
    reps = []
    for k, p in enumerate([7] + EDGE_PEERS):
        r = wire.Replica(p)
        child = r.map_set_container("m", "k%d" % (k % 4), wire.KIND_TEXT if k % 2 == 0 else wire.KIND_LIST)       # every child is (p, 0)
        if k % 2 == 0:
            r.text_insert(child, 0, "p%d" % k + ASTRAL); r.text_delete(child, 1, 1)
        else:
            r.list_insert(child, 0, [k, k + 1, k + 2]); r.list_delete(child, 0, 1)
        r.commit()
        reps.append(r)
    docs.append(Doc("children (p, 0) of six peers", reps))

    def names(r):
        for k, name in enumerate(["a", "ab", "abc", "name1", "name2", "n" * 300, "n" * 299 + "m", "名前é" + ASTRAL, "名前e"]):
            r.text_insert(name, 0, "q" * (k + 1) + str(k)); r.text_delete(name, k, 1)
            r.list_insert(name + "~", 0, [k] * (k + 2))
    docs.append(_one("names", 68, names))
    return docs


def peer_docs():
    """the id lookup (the binary search over the peer table, `qpid - id0 < ln`): documents of 1, 2 and 255 peers; `peer_queries` asks
    peers below, between and above the stored ones and the counter limits"""
    docs = [_one("one peer", 1 << 32, lambda r: (r.text_insert("text", 0, "solo"), r.text_delete("text", 1, 1)))]
    a, b = wire.Replica((1 << 63) - 1), wire.Replica(1 << 63)
    a.text_insert("text", 0, "left"); a.commit()                  # peer index 0 ends at its last counter in the Text …
    b.list_insert("list", 0, [1, 2]); b.commit()                   # … and (peer index 1, 0) lives in the List
    docs.append(Doc("two peers", [a, b]))
    reps = []
    for k in range(255):
        r = wire.Replica(1000 + 3 * k if k < 250 else EDGE_PEERS[k - 250])
        r.text_insert("text", 0, "%c" % (97 + k % 26) if k % 5 else ASTRAL)
        if k % 7 == 0:
            r.text_delete("text", 0, 1)
        r.commit()
        reps.append(r)
    docs.append(Doc("255 peers", reps))
    return docs


def peer_queries(doc, d):
    """lm_cursor_pos queries of `d`'s first container with ids no element has -> (pq, pw): ID_NOT_FOUND, all of them"""
    ex = Expect(d.model, sequence_cids(d.model)[0])
    peers = sorted({p for p, _ in d.model.all_ids})
    ask = {0, peers[0] - 1, peers[-1] + 1 if peers[-1] + 1 < 1 << 64 else 5, (1 << 32) - 1, (1 << 32) + 1, (1 << 63) - 2, (1 << 63) + 1, (1 << 64) - 2}
    ask |= {p + 1 for p in peers[:3]} | {p - 1 for p in peers[-3:]}
    pq = []
    for p in sorted(x for x in ask if 0 <= x < 1 << 64 and x not in peers):
        pq += [(doc, ex.key, (p, 0), MIDDLE), (doc, ex.key, (p, 1), LEFT)]
    for p in peers[:2] + peers[-2:]:
        for c in ((1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 1, -1, -(1 << 31)):
            pq.append((doc, ex.key, (p, c), RIGHT))
    other = [i for c in sequence_cids(d.model)[1:] for i in d.model.sequence_ids(c)]
    pq += [(doc, ex.key, i, MIDDLE) for i in other[:4]]
    pw = [ex.pos_answer(q[2], q[3]) for q in pq]
    assert all(w[0] == NOT_FOUND for w in pw)
    return pq, pw


def unreachable_child_case():
    """a child Text whose Map key is overwritten: answered like any other container (module docstring) — literals"""
    r = wire.Replica(5)
    child = r.map_set_container("m", "k", wire.KIND_TEXT)                               # (5, 0)
    r.text_insert(child, 0, "abc"); r.text_delete(child, 1, 1); r.map_set("m", "k", 1)  # a1 b2 c3, the delete is (5, 4), the overwrite (5, 5)
    empty = r.map_set_container("m", "e", wire.KIND_TEXT)                               # (5, 6): a child that never receives an op
    r.commit()
    key, ekey = cid_str(child), cid_str(empty)
    pq = [(0, key, (5, 1), MIDDLE), (0, key, (5, 2), RIGHT), (0, key, (5, 3), LEFT), (0, key, None, RIGHT), (0, key, (5, 5), MIDDLE)]
    pw = [(OK, 0, 0, MIDDLE), (DELETED, 1, 1, LEFT), (OK, 1, 1, LEFT), (OK, 2, 2, RIGHT), (NOT_FOUND, 0, 0, MIDDLE)]
    aq = [(0, key, 1, LEFT), (0, key, 2, MIDDLE)]
    aw = [(OK, (5, 3), LEFT, 1), (OK, None, RIGHT, 2)]
    return Doc("unreachable child", [r]), pq, pw, aq, aw, ekey


def empty_container_case():
    """A container that holds NO element at the rendered version: an entry checked out in front of the container's first op.
    `nr == 0` itself cannot be reached by k_cursor: the integrate kernels visit every Text / List row of the container table and
    start each tracker with one empty leaf (lm_k_integrate.h:706, lm_k_integrate_span.h:1777 `t.n_dir = 1`; the linear prefix keeps
    `w ? w : 1`, lm_k_integrate_linear.h:244; a resumed record with nr == 0 is an error, lm_k_integrate_span.h:1766), a document whose
    integrate stage failed is answered DOC_FAILED before the walk, and a key outside the table is CONTAINER_NOT_FOUND.  What can be
    built is nr == 1 with nothing in the leaf (`total == 0` in every pass).  -> (Doc, frontiers, pq, pw, aq, aw): literals"""
    r = wire.Replica(70)
    r.text_insert("a", 0, "x"); r.commit()                                   # (70, 0)
    r.text_insert("b", 0, "yz"); r.list_insert("c", 0, [1]); r.commit()      # (70, 1..2), (70, 3)
    d = Doc("empty containers", [r], [("in front of b and c", [(70, 0)])])
    B, C = "cid:root-b:Text", "cid:root-c:List"
    pq = [(0, B, (70, 1), MIDDLE), (0, B, None, RIGHT), (0, B, None, LEFT), (0, C, (70, 3), RIGHT), (0, C, None, MIDDLE), (0, "cid:root-a:Text", (70, 0), LEFT)]
    pw = [(NOT_FOUND, 0, 0, MIDDLE), (OK, 0, 0, RIGHT), (OK, 0, 0, LEFT), (NOT_FOUND, 0, 0, RIGHT), (OK, 0, 0, MIDDLE), (OK, 0, 0, LEFT)]
    aq = [(0, B, 0, MIDDLE), (0, B, 3, RIGHT), (0, C, 0, LEFT)]
    aw = [(OK, None, LEFT, 0), (OK, None, RIGHT, 0), (OK, None, LEFT, 0)]
    return d, [(70, 0)], pq, pw, aq, aw


def boundary_docs():
    return window_docs() + leaf_docs() + container_docs() + peer_docs()


# ------------------------------------------------------------------------------------------------ documents that arrive in steps
STEP_SEEDS = {"flat": 10, "text": 10, "nested": 10, "movable": 0}
STEP_FLOORS = {"pending_steps": 20, "renumbering_steps": 20}


def step_docs():
    """the six-step sessions of _merge_docs_steps (flat, text, nested; its writers, its deliveries) and its Text documents whose later
    steps bring peers that sort in front of, between and behind the stored ones around 2^32 and 2^63"""
    import _merge_docs_steps
    corp = _merge_docs_steps.step_corpora(STEP_SEEDS)
    return [d for name in ("flat", "text", "nested") for d in corp[name]] + [d.padded(6) for d in _merge_docs_steps.new_peer_docs("text")]


def step_counts(docs):
    import _merge_docs_steps
    tot = dict.fromkeys(STEP_FLOORS, 0)
    for d in docs:
        tot["pending_steps"] += sum(1 for ids in d.pending_ids if ids)
        tot["renumbering_steps"] += sum(_merge_docs_steps.renumbered(d))
    return tot


def run_steps(ctx, docs, what="steps"):
    """every step of every session as one batch: import, stand at the latest version, ask; then stand at the step's checkout, ask.
    The ids of the atoms that are delivered but pending are asked of every container.  -> the queries compared"""
    n = len(docs[0].steps)
    assert all(len(d.steps) == n for d in docs)
    ws = [d.wire_steps() for d in docs]
    sessions = [_merge_ref.Session(d.changes) for d in docs]
    total = 0
    for k in range(n):
        blobs = [w[k][0] for w in ws]
        if k == 0:
            ctx.stage(blobs, None)
            ctx.import_more([[] for _ in docs], None)          # resident from the first run on
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
            pq, pw, aq, aw = [], [], [], []
            for i, (d, s) in enumerate(zip(docs, sessions)):
                fr = frs[i] if sub else None
                if sub and fr is None:
                    continue
                a, b, c, e, xs = document_queries(i, s.model, fr)
                pending = sorted(d.pending_ids[k])
                for ex in xs:
                    for id_ in pending[:4] + pending[-4:]:
                        a.append((i, ex.key, id_, MIDDLE)); b.append((NOT_FOUND, 0, 0, MIDDLE))
                pq += a; pw += b; aq += c; aw += e
            total += check(ctx, pq, pw, aq, aw, "%s, step %d%s" % (what, k, " checked out" if sub else ""))
    return total


# ------------------------------------------------------------------------------------------------------- versions, three ways
def run_resident_versions(ctx, docs, what="resident"):
    """`docs` as resident documents: lm_stage + lm_run, then every version by an lm_import that brings nothing (k_cursor's at_version
    path: a future element is ID_NOT_FOUND).  The expected values are a Session's: a root shown once stays shown"""
    ctx.stage([d.blobs for d in docs]); ctx.run()
    sessions = [_merge_ref.Session(d.changes) for d in docs]
    want = [s.step(d.changes, None) for s, d in zip(sessions, docs)]
    total = 0
    for v in range(max(len(d.versions) for d in docs)):
        frs = [d.versions[v][1] if v < len(d.versions) else None for d in docs]
        if v:
            ctx.import_more([[] for _ in docs], [None if fr is None else wire.encode_frontiers(fr) for fr in frs]); ctx.run()
            want = [s.step([], fr) for s, fr in zip(sessions, frs)]
        got = ctx.fetch()
        pq, pw, aq, aw = [], [], [], []
        for i, (d, fr) in enumerate(zip(docs, frs)):
            assert got[i] == want[i], (what, d.label, v, got[i], want[i])
            if v < len(d.versions):
                a, b, c, e, _ = document_queries(i, d.model, fr)
                pq += a; pw += b; aq += c; aw += e
        total += check(ctx, pq, pw, aq, aw, "%s, version %d" % (what, v))
    return total


# ------------------------------------------------------------------------------------------------------------ query chunks and groups
def chunk_queries(doc, d):
    """63 / 64 / 65 / 129 queries on one container and one query 70 times -> [(pq, pw)], one call each"""
    ex = Expect(d.model, sequence_cids(d.model)[0])
    rng = random.Random(len(ex.order))
    out = []
    for n in (63, 64, 65, 129):
        pq = [(doc, ex.key, rng.choice(ex.order), rng.choice(SIDES)) for _ in range(n)]
        out.append((pq, [ex.pos_answer(q[2], q[3]) for q in pq]))
    tomb = [i for i in ex.order if i not in ex.vis] or ex.order
    q = (doc, ex.key, tomb[len(tomb) // 2], RIGHT)
    out.append(([q] * 70, [ex.pos_answer(q[2], q[3])] * 70))
    return out


def shuffled(pq, pw, aq, aw, seed=1):
    """the same queries in an order that mixes documents and containers: each answer is expected at its own index"""
    rng = random.Random(seed)
    a, b = list(range(len(pq))), list(range(len(aq)))
    rng.shuffle(a); rng.shuffle(b)
    return [pq[i] for i in a], [pw[i] for i in a], [aq[i] for i in b], [aw[i] for i in b]


def too_many_roots_doc():
    """65 root containers: beyond MAX_ROOTS (lm_types.h), the document is LM_UNSUPPORTED and so is every cursor on it"""
    return _one("65 roots", 69, lambda r: [r.text_insert("t%03d" % k, 0, "x") for k in range(65)])
