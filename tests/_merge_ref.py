"""A PLAIN model of what a merge computes: where concurrent inserts land, which elements a delete hits, who wins a map key,
what a checkout shows.  No oracle, kernel, decoder or tracker code: no runs, no leaves, no retreat / forward, no LCA, no cut.
It is small and slow and meant to be read as the definition.  Input: the writers' Change / Op objects (loro_amd.wire,
`_richtext_ref.changes_of(reps)`).  Output: the deep value as canonical JSON bytes (`_values.to_json`), the version vector
(`wire.encode_vv`) and the visible element ids of every Text / List.

Versions.  A version is a SET of op ids (peer, counter).  The version an op is applied on is the closure of its change's deps
plus the change's own atoms in front of the op (diff_calc.rs:480-481); the closure is computed by recursion over `deps`,
memoised per change.  Changes are processed by (lamport, peer, counter), a linear extension of the causal order.

Text / List.  One Python list per container holds every element ever inserted, in sequence order; an element knows its id,
its origin_left, its origin_right and the ids of the delete atoms that hit it.  An element is VISIBLE at a version P iff its id
is in P and none of its deleters is.  An insert atom at position `pos`, applied on version P (crdt_rope.rs:63-237):
  - origin_left = the visible element at pos - 1 (None at 0)                                        (crdt_rope.rs:84-108)
  - origin_right = the first element behind origin_left that is IN P, tombstones included (None if there is none); the
    elements between the two are all outside P ("future")                                           (crdt_rope.rs:110-146)
  - the atom is placed among those by the sibling rule, crdt_rope.rs:158-237, restated literally in `_place`.
  - "parent right" of (left, right) = the position of `right` iff right's own origin_left == left   (crdt_rope.rs:121-140, :197-210)
  The atoms of one insert op go through the rule one by one: atom k > 0 finds atom k - 1 at pos + k - 1 as its origin_left and
  the op's origin_right as its own, which is what a split run holds in the reference (fugue_span.rs Sliceable).
  A style_start is an element at `pos`; its style_end is an element at min(pos + mark_len + 1, visible length)
  (diff_calc.rs:1105-1132 "need to shift 1 because we insert the start style anchor before this pos").

Deletes are resolved by position: the targets are the |signed_len| elements visible at P from DeleteSpan::start
(list_op.rs:303-309, wire._del_start); atom i hits target i, of a reversed span (signed_len < 0) target n-1-i
(DeleteSpanWithId::slice, list_op.rs:251-277).  The writer recorded the ids it meant (op.del_id…): the model asserts them,
so a wrong view surfaces at the op that used it.

Map.  Per key the entry with the greatest (lamport, peer) wins (delta/map_delta.rs:26-32), lamport = change.lamport +
op.counter - change.counter; a map_delete competes like a write and removes the key (map_state.rs:438-449).

Child containers.  A child is part of the value where the list element / the winning map entry that created it is visible
(state.rs:1294-1329 get_deep_value resolves LoroValue::Container through the parent's value); its id is the creating op's id.

Root containers (diff_calc.rs:299 `!diff.is_empty() || bring_back`, state.rs:1352-1391; docs/ of the reference, "container
states are created lazily"): a document is imported (diff ∅ → latest) and then, for a checkout, taken to the version (diff
latest → version); a container state, once created, stays.  So a root Text / List is shown iff something is visible in it at
the latest version or at the checked-out one, a root Map iff the history holds an op for it (a deleted key is still an entry of
the diff, diff_calc.rs:553-605).

MovableList (diff_calc.rs:1669-1984, tracker.rs:289-347, state/movable_list_state.rs, handler.rs:3528-4000).  Its sequence holds
ITEMS; an ELEMENT is named by the IdLp (peer, lamport) of the insert atom that made it.
  - insert: a list_insert of n values places n items by `_place`; atom i has the item id (peer, counter + i) and makes the element
    (peer, lamport + i).  (The writer emits one op per value, handler.rs:3552-3585; encoding fuses contiguous ones.)
  - delete: the by-position rule above over the ITEMS visible at the op's version, whether an element still points at them or not.
  - move: a list_move with id (peer, c) at version P does two things under ONE id (tracker.rs:307-336): it deletes the item visible at
    P at position `move_from` (the model asserts that this item belongs to the element the writer named), and it places a new item
    with the id (peer, c), pointing at the same element, at position `pos` among the items visible after that delete — tombstones,
    the one just made included, still count as "in P" for the origin_right search.  As (peer, c) is both the deleter and the new
    item's id, `_place(els, P | {(peer, c)}, pos, …)` says exactly this.
  - set: a list_set touches no item.
  - the value at a version V: walk the items visible at V in sequence order; an item is shown iff it is the item of its element's
    greatest candidate by (lamport, peer id) among the insert and the moves whose id is in V (last_pos, history_cache.rs:754-1003);
    the element's value is that of its greatest candidate by (lamport, peer id) among the insert and the sets in V (last_value).
    A container value resolves to the child whose id is the creating op's id: the insert atom's, or the set op's.
  - a root MovableList is shown at EVERY version, empty or not, once the history holds an op for it (its diff lists every element the
    history knows, delta/movable_list.rs:32-34, diff_calc.rs:1880-1924) — unlike a root List.

Checkout: the same functions over the closure of the given frontiers.

Pending changes (oplog/pending_changes.rs; `Model(changes, delivered=…)`).  Of the changes that were DELIVERED a change applies iff
its peer's previous counter is applied (or it starts at 0) and every id it depends on lies in an applied change — the least fixpoint
of that rule, whatever the order of delivery.  The value and the version vector come from the applied changes only; the fourth element
of `result()` is the number of atoms delivered but not applied.  Pending does NOT depend on the checked-out version: the whole
history is imported first and the checkout follows (loro.rs import, then checkout), so a checkout of the applied part reports the
same count as the latest version.  Scope: no pending change is delivered twice (its atoms would be
counted once here) — duplicate only blobs that apply; the applied end of a peer lies on an op boundary of the writers' changes.

Map outcomes (`Model.map_outcomes`): what the LWW rule had to decide in this history, counted from the entries and the closures alone.

Documents that arrive in steps (`Session`; loro.rs:568-649 import on an attached document, loro.rs:1625-1760 checkout, diff_calc.rs:299,
state.rs:621-849).  A session holds the writers' changes of the whole history; `step(delivered_now, frontiers)` delivers some more of
them and renders.  After a step the applied set is `Model(changes, delivered=everything delivered so far)`: pending changes carry over
and resolve when their dependencies arrive — the model is rebuilt at every step, it is the definition and no fast path.  Every step
STANDS AT two versions in order: the latest version after its import, then the checked-out one if it has one (an import into a
checked-out document first returns to the latest version).  A container state, once created, stays (state.rs:621-849 never drops one):
a root Text / List is shown from the first stood-at version on in which something in it is visible (a step that brings an insert
together with its delete never shows it, a later step that empties it does not hide it again); a root Map is shown once an applied change
holds an op for it, a root MovableList likewise, at every version.  `Model.value(frontiers, shown=…)` takes the sticky set; without it
the rule of "Root containers" above (ONE import of everything, one checkout) holds.  Scope as above: no damaged input, no pending
change delivered twice, and a step never fails — every checkout version lies inside the applied set of its step.
A document that starts from a snapshot's STATE is the same session: it stands at the base version first and then takes the updates
(`Session.step` with the base's changes, then with the rest).  Only the expected values are the model's; the state section's bytes are
still written by the oracle's state writer (`_oracle.state_entries`).

Cross-step outcomes (`Model(…, step_of=…)`, `Model.cross`): OUTCOMES counted only where the rule compared two elements delivered in
DIFFERENT steps — "inserts": one of the atom's origins, "between": one of the elements between them, every other kind: the sibling
the rule looked at.

NOT modelled: Tree, Counter, damaged input, the BYTES of a snapshot's state section (a Python state writer; expected values are modelled).
"""
from _values import to_json
from loro_amd import wire

OUTCOMES = ("inserts", "between", "foreign_left_break", "same_right_break", "same_right_pass", "diff_right_less", "diff_right_greater",
            "diff_right_equal")
# what the element rules of a MovableList decided, at the latest version (Model.movable_outcomes)
# what the LWW rule of a Map decided (Model.map_outcomes)
MAP_OUTCOMES = ("concurrent_keys", "tie_on_lamport", "tie_won_by_last_delivered", "tie_won_by_first_delivered", "winner_is_delete",
                "child_map_hidden", "checkout_winner_differs")
MOVABLE_OUTCOMES = ("concurrent_moves", "winner_has_smaller_peer", "move_tie_on_lamport", "loser_item_alive", "winner_deleted_loser_alive",
                    "concurrent_sets", "set_tie_on_lamport")


class Elem:
    __slots__ = ("id", "origin_left", "origin_right", "deleters", "what")

    def __init__(self, id, origin_left, origin_right, what):
        self.id, self.origin_left, self.origin_right, self.what = id, origin_left, origin_right, what
        self.deleters = []


class Element:
    """a MovableList element: its candidates (lamport, peer, op id[, value]) for the position and for the value"""
    __slots__ = ("insert", "moves", "sets")

    def __init__(self, insert):
        self.insert, self.moves, self.sets = insert, [], []


def _greatest(cands):
    return max(cands, key=lambda c: (c[0], c[1]))


def _visible(e, P):
    if e.id not in P:
        return False
    for d in e.deleters:
        if d in P:
            return False
    return True


def _nth_visible(els, P, n):
    """index in `els` of the element at visible position `n` of version P, -1 if the visible length is not beyond n"""
    for i, e in enumerate(els):
        if _visible(e, P):
            if n == 0:
                return i
            n -= 1
    return -1


def _index_of(els, id):
    for i, e in enumerate(els):
        if e.id == id:
            return i
    raise KeyError(id)


def _parent_right(els, left, right):
    """crdt_rope.rs:121-140 / :197-210: the position of `right`, iff right's own origin_left is `left`"""
    if right is None:
        return None
    i = _index_of(els, right)
    return i if els[i].origin_left == left else None


def _cmp_pos(a, b):
    """crdt_rope.rs:453-466, Some < None"""
    if a is not None and b is not None:
        return (a > b) - (a < b)
    if a is not None:
        return -1
    if b is not None:
        return 1
    return 0


def _place(els, P, pos, id, what, stats, step_of=None, cross=None):
    """insert one element at visible position `pos` of version P.  `step_of` / `cross`: id -> delivery step, and the counts of the
    decisions that compared two elements of different steps"""
    def hit(kind, others):
        stats[kind] += 1
        if step_of is not None and any(o is not None and step_of[o] != step_of[id] for o in others):
            cross[kind] += 1
    left_at = -1
    if pos > 0:
        left_at = _nth_visible(els, P, pos - 1)
        assert left_at >= 0, ("insert position beyond the visible length", id, pos)
    origin_left = els[left_at].id if left_at >= 0 else None
    right_at = left_at + 1
    while right_at < len(els) and els[right_at].id not in P:
        right_at += 1
    origin_right = els[right_at].id if right_at < len(els) else None
    between = range(left_at + 1, right_at)
    hit("inserts", (origin_left, origin_right))
    insert_at = left_at + 1
    if len(between):
        hit("between", [els[i].id for i in between])
        mine = _parent_right(els, origin_left, origin_right)
        scanning, visited = False, set()
        for i in between:
            o = els[i]
            if o.origin_left != origin_left and (o.origin_left is None or o.origin_left not in visited):
                hit("foreign_left_break", (o.id,))
                break
            visited.add(o.id)
            if o.origin_left == origin_left:
                if o.origin_right == origin_right:
                    if o.id[0] > id[0]:
                        hit("same_right_break", (o.id,))
                        break
                    hit("same_right_pass", (o.id,))
                    scanning = False
                else:
                    c = _cmp_pos(_parent_right(els, origin_left, o.origin_right), mine)
                    if c < 0:
                        hit("diff_right_less", (o.id,))
                        scanning = True
                    elif c == 0:
                        hit("diff_right_equal", (o.id,))
                        if o.id[0] > id[0]:
                            break
                        scanning = False
                    else:
                        hit("diff_right_greater", (o.id,))
                        scanning = False
            if not scanning:
                insert_at = i + 1
    els.insert(insert_at, Elem(id, origin_left, origin_right, what))


def applied_ends(delivered):
    """peer -> first counter that is NOT applied, of the delivered changes (anything with peer / counter / ctr_end / deps): the least
    fixpoint of "its peer's previous counter is applied or it starts at 0, and every dep id lies in an applied change" """
    end = {}
    todo = list(delivered)
    progress = True
    while progress:
        progress = False
        rest = []
        for c in todo:
            have = end.get(c.peer, 0)
            if c.ctr_end <= have:
                continue                                    # known already: dropped
            if c.counter <= have and all(end.get(p, 0) > k for p, k in c.deps):
                end[c.peer] = c.ctr_end                     # (a change that overlaps the applied end is sliced: its tail applies)
                progress = True
            else:
                rest.append(c)
        todo = rest
    return end


def _cut(ch, end):
    """the ops of `ch` below the applied end `end` of its peer (an op boundary)"""
    if ch.ctr_end <= end:
        return ch
    ops = [o for o in ch.ops if o.counter + o.atom_len <= end]
    assert ops and ops[-1].counter + ops[-1].atom_len == end, ("the applied end of a peer cuts an op", ch.peer, end)
    return wire.Change(ch.peer, ch.counter, ch.lamport, list(ch.deps), ops, timestamp=ch.timestamp, msg=ch.msg)


class Model:
    def __init__(self, changes, delivered=None, step_of=None):
        """`changes`: the writers' changes.  `delivered`: the changes the document's blobs hold, when they are not all of them.
        `step_of`: id -> the step that delivered it (a session): `cross` counts the sibling decisions between different steps"""
        self.pending = 0
        self.step_of = step_of
        self.cross = {k: 0 for k in OUTCOMES}
        if delivered is not None:
            delivered = list(delivered)
            end = applied_ends(delivered)
            ids = {(c.peer, k) for c in delivered for k in range(c.counter, c.ctr_end)}
            self.pending = sum(1 for p, k in ids if k >= end.get(p, 0))
            changes = [_cut(c, end[c.peer]) for c in changes if c.counter < end.get(c.peer, 0)]
        self.changes = sorted(changes, key=lambda c: (c.lamport, c.peer, c.counter))
        self.by_peer = {}
        for c in self.changes:
            self.by_peer.setdefault(c.peer, []).append(c)
        for chs in self.by_peer.values():
            chs.sort(key=lambda c: c.counter)
        self._below = {}          # (peer, counter of a change) -> frozenset: the closure of its deps
        self.seqs = {}            # cid -> [Elem] in sequence order
        self.maps = {}            # cid -> key -> [(lamport, peer, op id, value or _GONE)]
        self.elems = {}           # MovableList cid -> element (peer, lamport) -> Element
        self.stats = {k: 0 for k in OUTCOMES}
        self.all_ids = frozenset((c.peer, k) for c in self.changes for k in range(c.counter, c.ctr_end))
        for c in self.changes:
            self._apply(c)

    # ---- versions
    def _change_of(self, id):
        for c in self.by_peer.get(id[0], ()):
            if c.counter <= id[1] < c.ctr_end:
                return c
        raise KeyError(id)

    def below(self, ch):
        """closure of the deps of `ch` (and of its peer's earlier changes: a peer's ops are a chain)"""
        key = (ch.peer, ch.counter)
        if key not in self._below:
            deps = list(ch.deps) + ([(ch.peer, ch.counter - 1)] if ch.counter > 0 else [])
            self._below[key] = frozenset().union(*[self.closure_of_id(d) for d in deps])
        return self._below[key]

    def closure_of_id(self, id):
        ch = self._change_of(id)
        return self.below(ch) | {(ch.peer, k) for k in range(ch.counter, id[1] + 1)}

    def version(self, frontiers=None):
        """the set of ids of a checkout target; None = everything"""
        if frontiers is None:
            return self.all_ids
        return frozenset().union(*[self.closure_of_id(f) for f in frontiers])

    # ---- replay
    def _apply(self, ch):
        base = self.below(ch)
        for op in ch.ops:
            lam = ch.lamport + op.counter - ch.counter
            if op.kind in ("map_set", "map_delete"):      # (a Map write needs no version: its entry competes wherever it is seen)
                self.maps.setdefault(op.cid, {}).setdefault(op.key, []).append(
                    (lam, ch.peer, (ch.peer, op.counter), op.value if op.kind == "map_set" else _GONE))
                continue
            P = base | {(ch.peer, k) for k in range(ch.counter, op.counter)}
            els = self.seqs.setdefault(op.cid, [])
            if op.cid.kind == wire.KIND_MOVABLE and op.kind != "delete":
                self._apply_movable(ch, op, P, lam, els)
            elif op.kind == "text_insert":
                for i, c in enumerate(op.text):
                    _place(els, P | {(ch.peer, op.counter + k) for k in range(i)}, op.pos + i, (ch.peer, op.counter + i), ("char", c), self.stats, self.step_of, self.cross)
            elif op.kind == "list_insert":
                for i, v in enumerate(op.values):
                    _place(els, P | {(ch.peer, op.counter + k) for k in range(i)}, op.pos + i, (ch.peer, op.counter + i), ("value", v), self.stats, self.step_of, self.cross)
            elif op.kind == "style_start":
                _place(els, P, op.pos, (ch.peer, op.counter), ("start", op), self.stats, self.step_of, self.cross)
            elif op.kind == "style_end":
                start = next(e.what[1] for e in els if e.id == (ch.peer, op.counter - 1))
                n_visible = sum(1 for e in els if _visible(e, P))
                _place(els, P, min(start.pos + start.mark_len + 1, n_visible), (ch.peer, op.counter), ("end",), self.stats, self.step_of, self.cross)
            elif op.kind == "delete":
                n = abs(op.signed_len)
                first = wire._del_start(op)
                targets = [e for e in els if _visible(e, P)][first:first + n]
                assert len(targets) == n, ("delete beyond the visible length", (ch.peer, op.counter))
                assert [e.id for e in targets] == [(op.del_id[0], op.del_id[1] + j) for j in range(n)], \
                    ("the delete does not hit the ids its writer meant", (ch.peer, op.counter), op.del_id, [e.id for e in targets])
                for i in range(n):
                    targets[i if op.signed_len > 0 else n - 1 - i].deleters.append((ch.peer, op.counter + i))
            else:
                raise NotImplementedError(op.kind)

    def _apply_movable(self, ch, op, P, lam, els):
        elems = self.elems.setdefault(op.cid, {})
        id = (ch.peer, op.counter)
        if op.kind == "list_insert":
            for i, v in enumerate(op.values):
                assert (ch.peer, lam + i) not in elems
                elems[(ch.peer, lam + i)] = Element((lam + i, ch.peer, (ch.peer, op.counter + i), v))
                _place(els, P | {(ch.peer, op.counter + k) for k in range(i)}, op.pos + i, (ch.peer, op.counter + i), ("item", (ch.peer, lam + i)), self.stats, self.step_of, self.cross)
        elif op.kind == "list_move":
            at = _nth_visible(els, P, op.move_from)
            assert at >= 0, ("move from beyond the visible length", id)
            assert els[at].what == ("item", op.elem), ("the move does not take the element its writer meant", id, op.elem, els[at].what)
            els[at].deleters.append(id)
            elems[op.elem].moves.append((lam, ch.peer, id))
            _place(els, P | {id}, op.pos, id, ("item", op.elem), self.stats, self.step_of, self.cross)
        elif op.kind == "list_set":
            assert elems[op.elem].insert[2] in P, ("a set of an element its writer has not seen", id)
            elems[op.elem].sets.append((lam, ch.peer, id, op.value))
        else:
            raise NotImplementedError(op.kind)

    def movable_outcomes(self):
        """MOVABLE_OUTCOMES at the latest version: what the element rules had to decide in this history.  Per element —
        concurrent_moves: the causal closure of its winning move does not hold another of its moves; winner_has_smaller_peer: one
        of those has the greater peer id (the lamport decided); move_tie_on_lamport: one of those has the winner's lamport (the
        peer id decided); winner_deleted_loser_alive: the item of its winner is deleted, another item of its is alive;
        concurrent_sets / set_tie_on_lamport: the same over its sets.  Per item — loser_item_alive: alive, and no element's
        winner."""
        tot = dict.fromkeys(MOVABLE_OUTCOMES, 0)
        for cid, elems in self.elems.items():
            alive = {e.id: e.what[1] for e in self.seqs[cid] if _visible(e, self.all_ids)}
            pointed = set()
            for name, el in elems.items():
                win = _greatest([el.insert[:3]] + el.moves)
                pointed.add(win[2])
                others = [m for m in el.moves if m[2] != win[2] and m[2] not in self.closure_of_id(win[2])]
                if others:                           # a move the winner had not seen: (lamport, peer id) decided
                    tot["concurrent_moves"] += 1
                    tot["winner_has_smaller_peer"] += any(m[1] > win[1] for m in others)
                    tot["move_tie_on_lamport"] += any(m[0] == win[0] for m in others)
                if win[2] not in alive and name in alive.values():
                    tot["winner_deleted_loser_alive"] += 1
                if el.sets:
                    win = _greatest(el.sets)
                    others = [m for m in el.sets if m[2] != win[2] and m[2] not in self.closure_of_id(win[2])]
                    if others:
                        tot["concurrent_sets"] += 1
                        tot["set_tie_on_lamport"] += any(m[0] == win[0] for m in others)
            tot["loser_item_alive"] += sum(1 for id in alive if id not in pointed)
        return tot

    def map_winner(self, cid, key, V):
        """the winning entry (lamport, peer, op id, value) of a key at the version V, None if V holds no write to it"""
        seen = [e for e in self.maps[cid][key] if e[2] in V]
        return max(seen, key=lambda e: (e[0], e[1])) if seen else None

    def map_pairs(self, frontiers=None):
        """the number of distinct (Map, key) pairs the version holds a write to"""
        V = self.version(frontiers)
        return sum(1 for keys in self.maps.values() for entries in keys.values() if any(e[2] in V for e in entries))

    def map_outcomes(self, delivery=(), versions=()):
        """MAP_OUTCOMES, per (Map, key), at the latest version.  concurrent_keys: the closure of the winner's id does not hold another
        write to the key (the rule, not causality, decided); tie_on_lamport: one of those has the winner's lamport (the peer id
        decided); tie_won_by_last_delivered / _first_delivered: `delivery` lists the peers in the order their blobs are delivered, and
        the winner of such a tie comes after / before every peer it tied with; winner_is_delete; child_map_hidden: per child Map whose
        creating write lost to a write that had not seen it; checkout_winner_differs: at one of `versions` (frontiers) the key has a
        winner, and it is not the latest one."""
        tot = dict.fromkeys(MAP_OUTCOMES, 0)
        rank = {p: i for i, p in enumerate(delivery)}
        Vs = [self.version(fr) for fr in versions]
        for cid, keys in self.maps.items():
            for key, entries in keys.items():
                win = self.map_winner(cid, key, self.all_ids)
                below = self.closure_of_id(win[2])
                others = [e for e in entries if e[2] != win[2] and e[2] not in below]
                if others:
                    tot["concurrent_keys"] += 1
                    tied = [e for e in others if e[0] == win[0]]
                    if tied:
                        tot["tie_on_lamport"] += 1
                        if win[1] in rank and all(e[1] in rank for e in tied):
                            tot["tie_won_by_last_delivered"] += all(rank[win[1]] > rank[e[1]] for e in tied)
                            tot["tie_won_by_first_delivered"] += all(rank[win[1]] < rank[e[1]] for e in tied)
                tot["winner_is_delete"] += win[3] is _GONE
                tot["child_map_hidden"] += sum(1 for e in others if isinstance(e[3], wire.ContainerValue) and e[3].kind == wire.KIND_MAP)
                for V in Vs:
                    w = self.map_winner(cid, key, V)
                    if w is not None and w[2] != win[2]:
                        tot["checkout_winner_differs"] += 1
                        break
        return tot

    # ---- reading
    def visible_ids(self, cid, frontiers=None):
        V = self.version(frontiers)
        return [e.id for e in self.seqs.get(cid, ()) if _visible(e, V)]

    def sequence_ids(self, cid):
        """every element ever inserted, in sequence order (an order that does not depend on the version)"""
        return [e.id for e in self.seqs.get(cid, ())]

    def sequences(self):
        return list(self.seqs)

    def _value(self, cid, V):
        if cid.kind == wire.KIND_MAP:
            out = {}
            for key, entries in self.maps.get(cid, {}).items():
                seen = [e for e in entries if e[2] in V]
                if seen:
                    lam, peer, id, v = max(seen, key=lambda e: (e[0], e[1]))
                    if v is not _GONE:
                        out[key] = self._resolve(v, id, V)
            return out
        els = [e for e in self.seqs.get(cid, ()) if _visible(e, V)]
        if cid.kind == wire.KIND_MOVABLE:
            out = []
            for e in els:
                el = self.elems[cid][e.what[1]]
                if _greatest([el.insert[:3]] + [m for m in el.moves if m[2] in V])[2] == e.id:      # last_pos
                    lam, peer, id, v = _greatest([el.insert] + [s for s in el.sets if s[2] in V])   # last_value
                    out.append(self._resolve(v, id, V))
            return out
        if cid.kind == wire.KIND_TEXT:
            return "".join(e.what[1] for e in els if e.what[0] == "char")
        assert cid.kind == wire.KIND_LIST, cid
        return [self._resolve(e.what[1], e.id, V) for e in els]

    def _resolve(self, v, id, V):
        if isinstance(v, wire.ContainerValue):
            return self._value(wire.CID(False, v.kind, "", id[0], id[1]), V)
        return v

    def seen_roots(self, frontiers=None):
        """the root Text / List containers in which something is visible at the version"""
        V = self.version(frontiers)
        return {cid for cid, els in self.seqs.items() if cid.root and cid.kind != wire.KIND_MOVABLE and any(_visible(e, V) for e in els)}

    def value(self, frontiers=None, shown=None):
        """the deep value: root name -> plain Python value.  `shown`: the root Text / List containers whose state exists (a session's
        sticky set); None = one import of everything, then the checkout"""
        V = self.version(frontiers)
        if shown is None:
            shown = self.seen_roots() | self.seen_roots(frontiers)
        roots = {}
        for cid in list(self.seqs) + list(self.maps):
            if not cid.root:
                continue
            if cid.kind not in (wire.KIND_MAP, wire.KIND_MOVABLE) and cid not in shown:
                continue
            assert cid.name not in roots, "two root containers share a name"
            roots[cid.name] = self._value(cid, V)
        return roots

    def json(self, frontiers=None, shown=None):
        return to_json(self.value(frontiers, shown)).encode("utf-8")

    def vv(self, frontiers=None):
        out = {}
        for p, c in self.version(frontiers):
            out[p] = max(out.get(p, 0), c + 1)
        return wire.encode_vv(out)

    def result(self, frontiers=None, shown=None):
        """(status, json, vv, pending) as merge_batch returns it"""
        return (0, self.json(frontiers, shown), self.vv(frontiers), self.pending)


class Session:
    """a document delivered in steps (module docstring, "Documents that arrive in steps")"""

    def __init__(self, changes):
        self.changes = list(changes)
        self.delivered = []          # every change delivered so far, in the order of delivery
        self.step_of = {}            # id -> the step that delivered it first
        self.shown = set()           # root Text / List containers whose state exists
        self.n_steps = 0
        self.model = None            # the model of the applied set after the last step

    def step(self, delivered_now, frontiers=None):
        """deliver `delivered_now` (changes), stand at the latest version, then at `frontiers` if given -> (status, json, vv, pending)"""
        for c in delivered_now:
            self.delivered.append(c)
            for k in range(c.counter, c.ctr_end):
                self.step_of.setdefault((c.peer, k), self.n_steps)
        self.n_steps += 1
        m = self.model = Model(self.changes, delivered=self.delivered, step_of=self.step_of)
        self.shown |= m.seen_roots()
        if frontiers is not None:
            self.shown |= m.seen_roots(frontiers)
        return m.result(frontiers, self.shown)


_GONE = object()


# ---- a writer's view from the model: what `_fuzz.random_session(view=...)` takes instead of the oracle's refresh
def view(replica, cid):
    """visible ids of `cid` in everything `replica` holds (committed changes); of a MovableList the ids of its alive ITEMS, pointed at
    or not, in op-index order — what wire.Replica.mlist_* keeps in `seq`"""
    key = tuple(sorted(replica.vv.items()))
    cached = getattr(replica, "_merge_ref_view", None)
    if cached is None or cached[0] != key:
        cached = (key, Model([c for chs in replica.changes.values() for c in chs]))
        replica._merge_ref_view = cached
    return cached[1].visible_ids(cid)
