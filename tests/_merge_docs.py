"""Documents for the tests of the plain merge model (tests/_merge_ref.py): fuzz corpora whose writers take their view from the
model (no decision of the oracle in them), hand-built documents aimed at the edges of the integrate kernels, and the checkout
versions of each.  Shared by tests/test_merge_ref.py (oracle, kernel-logic harness) and tests/test_gpu_zz_merge_ref.py; the
MovableList documents (second half) by tests/test_merge_ref_movable.py and tests/test_gpu_zz_merge_ref_movable.py."""
import random

import _fuzz, _merge_ref
from _richtext_ref import changes_of
from loro_amd import wire

TEXT = wire.root_cid("text", wire.KIND_TEXT)
ML = wire.root_cid("ml", wire.KIND_MOVABLE)
V = _merge_ref.view


class Doc:
    """one document: its blobs, the model of it and the versions it is checked out at"""

    def __init__(self, label, reps, snaps=(), n_versions=4, blobs=None):
        self.label = label
        self.reps = reps
        self.snaps = [(list(fr), blob) for fr, blob in snaps]          # (frontiers, updates holding exactly that version or None)
        self.blobs = _fuzz.blobs_of(reps) if blobs is None else blobs
        self.model = _merge_ref.Model(changes_of(reps))
        rng = random.Random(len(self.blobs[0]) if self.blobs else 0)
        cuts = delete_run_cuts(self.model)
        ends = [[(c.peer, c.ctr_end - 1)] for c in self.model.changes]
        picks = [list(fr) for fr, _ in snaps]
        rng.shuffle(picks)
        self.cut_versions = [rng.choice(cuts)] if cuts else []
        self.versions = self.cut_versions + picks[:n_versions - 1] + ([rng.choice(ends)] if ends else [])


def delete_run_cuts(model):
    """frontiers that end inside a delete op of more than one atom: the version holds a part of the run"""
    out = []
    for c in model.changes:
        for op in c.ops:
            if op.kind == "delete" and abs(op.signed_len) >= 2:
                out.append([(c.peer, op.counter + (abs(op.signed_len) - 1) // 2)])
    return out


def _session(label, seeds, **kw):
    docs = []
    for s in seeds:
        snaps = []
        reps = _fuzz.random_session(s, snapshots=snaps, view=V, **kw)
        docs.append(Doc("%s seed %d" % (label, s), reps, snaps))
    return docs


def corpora():
    """name -> [Doc].  The sizes beyond the first corpus: the fewest seeds, in steps of ten, at which check_conditions holds"""
    out = {
        "3 peers": _session("3 peers", range(60), n_peers=3, n_steps=80, kinds=("text", "list")),
        "5 peers": _session("5 peers", range(100, 120), n_peers=5, n_steps=120, kinds=("text", "list"), sync_prob=0.05),
        "with map": _session("with map", range(200, 230), n_peers=3, n_steps=80, kinds=("text", "list", "map")),
        "styles": _session("styles", range(300, 330), n_peers=3, n_steps=80, kinds=("text", "list"), styles=True),
    }
    out["nested"] = []
    for s in range(400, 420):     # (nested_session records no versions: every fourth change's end is one)
        reps = _fuzz.nested_session(s, view=V)
        out["nested"].append(Doc("nested seed %d" % s, reps, [([(r.peer, ch.ctr_end - 1)], None) for r in reps for ch in r.changes.get(r.peer, [])[1::4]]))
    return out


def outcome_counts(docs):
    tot = dict.fromkeys(_merge_ref.OUTCOMES + _merge_ref.MOVABLE_OUTCOMES, 0)
    for d in docs:
        for k, v in list(d.model.stats.items()) + list(d.model.movable_outcomes().items()):
            tot[k] += v
    return tot


MOVABLE_AT_LEAST = {"concurrent_moves": 50, "winner_has_smaller_peer": 20, "move_tie_on_lamport": 1, "loser_item_alive": 50,
                    "winner_deleted_loser_alive": 10, "concurrent_sets": 50, "set_tie_on_lamport": 1}


def check_conditions(name, docs):
    """asserted from the model alone, before anything is compared: a corpus cannot pass by being boring"""
    tot = outcome_counts(docs)
    for k in _merge_ref.OUTCOMES:
        assert tot[k] >= (1 if k == "diff_right_equal" else 50), (name, k, tot)
    if any(d.model.elems for d in docs):          # a MovableList corpus: what the element rules decided, too
        for k, least in MOVABLE_AT_LEAST.items():
            assert tot[k] >= least, (name, k, tot)
    latest = {d.label: d.model.json() for d in docs}
    assert any(d.model.json(v) != latest[d.label] for d in docs for v in d.versions), name
    assert any(d.cut_versions for d in docs), name


# ------------------------------------------------------------------------------------------------------------ hand-built documents
def _sync(reps):
    for r in reps:
        r.commit()
    for a in reps:
        for b in reps:
            if a is not b and a.merge_from(b):
                pass
    for r in reps:
        for cid in {c for x in reps for c in x.seq}:
            r.set_visible(cid, cid.kind, V(r, cid))


def three_peer_text(n_runs, seed):
    """A base of `n_runs` runs written by one peer (a leaf of the span-granular tracker holds 64 items: 70 runs split one leaf, 130
    make three leaves, 300 more than LM_DIR_OPT_MAX=4 allows); then all three peers insert, concurrently, one character at EVERY
    run boundary — so in every leaf's first and last slot — and several times at one position; after a sync, a second round with
    deletes across the first round's siblings."""
    rng = random.Random(seed)
    a, b, c = (wire.Replica(p) for p in rng.sample(range(1, 1 << 30), 3))
    n = 0
    for i in range(n_runs):
        pos = n if i % 3 else rng.randint(0, n)
        a.text_insert("text", pos, "abcdefg"[:2 + i % 3]); n += 2 + i % 3
        if i % 3 == 0:
            a.text_delete("text", pos + 1, 1); n -= 1           # keeps appended runs from merging into one op
        if i % 40 == 0:
            a.commit()
    _sync([a, b, c])
    base = list(a.seq[TEXT])
    bounds = [i for i in range(1, len(base)) if base[i] != (base[i - 1][0], base[i - 1][1] + 1)]
    for r, ch in ((a, "A"), (b, "B"), (c, "C")):
        for k, at in enumerate(reversed(bounds)):              # right to left: the positions of the base stay valid
            r.text_insert("text", at, ch)
            if k % 50 == 0:
                r.commit()
        spot = bounds[len(bounds) // 2]
        for k in range(4):                                     # one position, several times: typed forward and backward
            r.text_insert("text", spot + (k if k % 2 else 0), ch.lower() * (1 + k))
        r.commit()
    _sync([a, b, c])
    for r in (a, b, c):
        ids = r.seq[TEXT]
        for k in range(6):
            pos = rng.randrange(len(ids) - 8)
            r.text_delete("text", pos, rng.randint(2, 6))
            r.text_insert("text", rng.randint(0, len(ids)), "xyz"[:1 + k % 3])
        r.commit()
    return Doc("three peers, %d runs" % n_runs, [a, b, c], [([(r.peer, ch.ctr_end - 1)], None) for r in (a, b, c) for ch in r.changes[r.peer][1::3]])


def sweep_docs():
    """Two peers; the second one's concurrent branch is `n` ids long, for every n from 65 to 144: k_integrate_span_plain_sweep moves a
    range of more than 8 x leaves + 64 ids by a pass over the leaves and a shorter one row by row — for every leaf count from 1 to 10
    one document lies just below its threshold (n = 8 x leaves + 64) and one just past it (n + 1)."""
    docs = []
    for n in range(65, 145):
        rng = random.Random(n)
        a, b = wire.Replica(1000 + n), wire.Replica(7)
        a.text_insert("text", 0, "0123456789" * 4); a.commit()
        _sync([a, b])
        used = 0
        while used < n:                                        # the branch: scattered inserts, typing, a few deletes
            ids = b.seq[TEXT]
            k = min(n - used, rng.randint(1, 3))
            if used % 7 == 3 and len(ids) > 4:
                b.text_delete("text", rng.randrange(len(ids) - k), k)
            else:
                b.text_insert("text", rng.randint(0, len(ids)), "bcd"[:k])
            used += k
            if rng.random() < 0.3:
                b.commit()
        b.commit()
        for k in range(5):                                     # the other branch, replayed after (or before) it
            a.text_insert("text", rng.randint(0, len(a.seq[TEXT])), "A" * (1 + k % 2))
            a.text_delete("text", rng.randrange(len(a.seq[TEXT]) - 2), 2)
            a.commit()
        _sync([a, b])
        a.text_insert("text", 3, "end"); a.commit()
        docs.append(Doc("branch of %d ids" % n, [a, b], [([(b.peer, b.changes[b.peer][-1].ctr_end - 1)], None)], n_versions=2))
    return docs


def linear_prefix_docs():
    """a single chain of about 300 steps by one replica, handed over to two (or three) concurrent branches"""
    out = []
    for s in range(6):
        snaps = []
        reps = _fuzz.random_session(500 + s, n_peers=2 + s % 2, n_steps=40, kinds=("text", "list")[:1 + s % 2], solo_steps=300, solo_peer=s % 2,
                                    max_del=[4, 40][s % 2], snapshots=snaps, view=V)
        out.append(Doc("linear prefix seed %d" % (500 + s), reps, snaps))
    return out


def id_window_docs():
    """loc[] keeps item heads and every 16th id of a run: one run of 100 ids, then concurrent inserts and deletes whose targets
    straddle the 16-aligned counters (…15|16…, …31|32…), from two peers; a second round after the sync."""
    out = []
    for s in range(8):
        rng = random.Random(900 + s)
        a, b, c = wire.Replica(50 + s), wire.Replica(20 + s), wire.Replica(90 + s)
        if s % 2:
            a.text_insert("text", 0, "x" * (s + 1))            # the long run does not begin at counter 0
        a.text_insert("text", 0, "".join(chr(97 + i % 26) for i in range(100))); a.commit()
        _sync([a, b, c])
        for rnd in range(2):
            for r in (b, c, a):
                for edge in rng.sample([16, 32, 48, 64, 80], 3):
                    ids = r.seq[TEXT]
                    pos = min(len(ids) - 4, max(0, edge + rng.randint(-2, 1)))
                    if rng.random() < 0.5:
                        r.text_delete("text", pos, rng.randint(1, 4))
                    else:
                        r.text_insert("text", pos, "IJ"[:rng.randint(1, 2)])
                    if rng.random() < 0.5:
                        r.commit()
                r.commit()
            _sync([a, b, c])
        out.append(Doc("id windows %d" % s, [a, b, c], [([(r.peer, ch.ctr_end - 1)], None) for r in (a, b, c) for ch in r.changes[r.peer][1::2]]))
    return out


def backspace_docs():
    """Backspacing merges into ONE delete op of negative length whose atoms hit their targets from right to left
    (DeleteSpan::merge, list_op.rs:396-423; DeleteSpanWithId::slice, :251-277); pressing Delete at one position merges into a
    forward one.  Three peers do both concurrently, over each other's targets; every document is checked out inside such a run."""
    out = []
    for s in range(8):
        rng = random.Random(1200 + s)
        reps = [wire.Replica(p) for p in rng.sample(range(1, 1 << 20), 3)]
        reps[0].text_insert("text", 0, "".join(chr(97 + i % 26) for i in range(60))); reps[0].commit()
        _sync(reps)
        cuts = []
        for rnd in range(3):
            for r in reps:
                for _ in range(2):
                    n = len(r.seq[TEXT])
                    k = rng.randint(2, 6)
                    pos = rng.randrange(k, n - k)
                    r.commit()
                    if rng.random() < 0.6:
                        for j in range(k):
                            r.text_delete("text", pos - j, 1)              # backspace
                    else:
                        for j in range(k):
                            r.text_delete("text", pos, 1)                  # forward delete
                    for op in r.pending_ops:    # (only id-contiguous targets merge: a run the others have not written into)
                        if abs(op.signed_len) >= 2:
                            cuts.append(([(r.peer, op.counter + rng.randrange(abs(op.signed_len) - 1))], None))
                    r.text_insert("text", rng.randint(0, len(r.seq[TEXT])), "XY"[:rng.randint(1, 2)])
                    r.commit()
            _sync(reps)
        rng.shuffle(cuts)
        d = Doc("backspace %d" % s, reps, cuts[:4], n_versions=6)
        assert any(op.kind == "delete" and op.signed_len <= -2 for c in d.model.changes for op in c.ops)
        out.append(d)
    return out


# ==================================================================================================================== MovableList
def movable_corpora():
    """name -> [Doc] from _fuzz.movable_session with the writers' views from the model.  Sizes: the fewest seeds, in steps of ten, at
    which check_conditions holds (what binds: winner_deleted_loser_alive >= 10 for the first and the third, reached at 90 seeds
    with 12 and 11; for the nested one at 50 seeds with 10)"""
    out = {}
    for name, seeds, kw in (("movable", range(100, 190), {}),
                            ("movable nested", range(200, 250), dict(nested=True, n_steps=160, n_peers=4)),
                            ("movable 5 peers", range(600, 690), dict(n_peers=5, n_steps=120, sync_prob=0.05))):
        out[name] = []
        for s in seeds:
            snaps = []
            reps = _fuzz.movable_session(s, snapshots=snaps, view=V, **kw)
            out[name].append(Doc("%s seed %d" % (name, s), reps, snaps))
    return out


def overlapping_docs(docs):
    """the same documents delivered as every replica's WHOLE export (as test_emu_movable.session_docs does): the histories overlap,
    known changes — move and set rows among them — are dropped or sliced on import"""
    out = []
    for d in docs:
        o = Doc.__new__(Doc)
        o.__dict__.update(d.__dict__)
        o.label, o.blobs = d.label + ", whole exports", [r.export() for r in d.reps]
        out.append(o)
    return out


def _ids_of(r, since=0):
    """[(frontiers, None)] at the end of each change of `r`'s own from its `since`-th on"""
    return [([(r.peer, ch.ctr_end - 1)], None) for ch in r.changes.get(r.peer, [])[since:]]


def _all_versions(label, reps, snaps, blobs=None):
    return Doc(label, reps, snaps, n_versions=len(snaps) + 1, blobs=blobs)


# peer ids of the lamport-tie documents: [the peer that makes the list] + the peers that move / set concurrently.  Every document is
# delivered twice, the competitors' blobs in the order given and in the reverse order, the list's maker last: numeric order differs
# from delivery order and from the order of first appearance in one of the two at least.  The last two sets have ids on both sides of
# 2^32 and of 2^63 (a signed or a truncated compare orders them differently).
TIE_PEERS = [[50, 70, 20], [50, 70, 60, 90], [50, 90, 20, 70], [(1 << 32) + 1, (1 << 63) + 5, (1 << 32) - 1, (1 << 63) - 1],
             [(1 << 63) - 2, 3, (1 << 64) - 9, (1 << 32) + 7]]


def lamport_tie_docs():
    """Two or three peers move — and, separately, set; and both — the SAME element concurrently from the same version: the candidates'
    lamports are equal and the peer id decides (last_pos / last_value compare (lamport, peer)).  Every document is also checked out
    at each competitor's op alone, at every pair of them and in front of them."""
    out = []
    for peers in TIE_PEERS:
        for what in ("move", "set", "both"):
            reps = [wire.Replica(p) for p in peers]
            reps[0].mlist_insert("ml", 0, ["a", "b", "c", "d", "e"]); reps[0].commit()
            base = list(reps[0].frontiers)
            _sync(reps)
            snaps = [(base, None)]
            for k, r in enumerate(reps[1:]):
                if what != "move":
                    r.mlist_set("ml", 2, "set by %d" % k)
                if what != "set":
                    r.mlist_move("ml", 1, [3, 0, 4][k])
                r.commit()
                snaps += [([(r.peer, c)], None) for c in range(r.changes[r.peer][0].ctr_end)]
            ends = [fr[0] for fr, _ in snaps[1:] if fr[0][1] == (1 if what == "both" else 0)]
            snaps += [([a, b], None) for i, a in enumerate(ends) for b in ends[i + 1:]]
            _sync(reps)
            reps[1].mlist_insert("ml", 2, ["after"]); reps[1].commit()
            d = _all_versions("lamport tie, %s, peers %s" % (what, peers), reps, snaps, blobs=[_own(r) for r in reps[1:]] + [_own(reps[0])])
            got = d.model.movable_outcomes()
            assert (what == "set" or got["move_tie_on_lamport"] == 1) and (what == "move" or got["set_tie_on_lamport"] == 1), (d.label, got)
            out += [d, _all_versions(d.label + ", delivered in reverse", reps, snaps, blobs=[_own(r) for r in reps[:0:-1]] + [_own(reps[0])])]
    return out


def _own(r):
    return _fuzz.blobs_of([r])[0]


def move_against_delete_docs():
    """(docs, the values they must have).  A moves an element while B deletes it concurrently: it survives at A's item.  B deletes it
    after seeing A's move M1 while C's concurrent move M2 is the smaller by (lamport, peer): the element is gone and M2's item stays
    alive with no element pointing at it; with M2 the greater one the element is shown at M2's item.  Later inserts and moves by
    position land around the unreferenced item."""
    docs, want = [], []
    a, b = wire.Replica(7), wire.Replica(4)
    a.mlist_insert("ml", 0, ["a", "b", "c", "d"]); a.commit()
    _sync([a, b])
    a.mlist_move("ml", 1, 3); a.commit()
    b.mlist_delete("ml", 1, 1); b.commit()
    snaps = _ids_of(a, 1) + _ids_of(b)
    _sync([a, b])
    b.mlist_insert("ml", 3, ["x"]); b.mlist_move("ml", 4, 0); b.commit()
    docs.append(_all_versions("move against a concurrent delete", [a, b], snaps + _ids_of(b, 1)))
    want.append(["b", "a", "c", "d", "x"])
    for pa, pc, shown in ((30, 20, False), (20, 30, True)):
        a, b, c = wire.Replica(pa), wire.Replica(25), wire.Replica(pc)
        a.mlist_insert("ml", 0, ["a", "b", "c", "d"]); a.commit()
        _sync([a, b, c])
        a.mlist_move("ml", 1, 3); a.commit()                  # M1: a c d b
        c.mlist_move("ml", 1, 0); c.commit()                  # M2: b a c d, the same lamport
        b.merge_from(a); b.set_visible(ML, ML.kind, V(b, ML))
        b.mlist_delete("ml", 3, 1); b.commit()                # deletes M1's item
        snaps = _ids_of(a, 1) + _ids_of(c) + _ids_of(b)
        snaps.append(([snaps[1][0][0], snaps[2][0][0]], None))
        _sync([a, b, c])
        for r, v in ((a, "A"), (c, "C")):                     # concurrently again: by position, around M2's item
            r.mlist_insert("ml", 0, [v + "0"]); r.mlist_insert("ml", 2, [v + "2"]); r.mlist_move("ml", r.mlist_len("ml") - 1, 0); r.commit()
        d = _all_versions("delete after M1, concurrent M2 is the %s" % ("greater" if shown else "smaller"), [a, b, c], snaps + _ids_of(a, 2) + _ids_of(c, 1))
        got = d.model.movable_outcomes()
        assert got["winner_deleted_loser_alive"] == (0 if shown else 1) and got["loser_item_alive"] >= 1, (d.label, got)    # (the second round leaves a loser, too)
        docs.append(d)
        want.append(None)
    return docs, want


def _raw_move(r, cid, items, elem, to):
    """a list_move row written straight from a list of (item id, element) kept beside the replica (wire.Replica.mlist_move rebuilds
    its element index from the whole history at every call); the model asserts that the row takes the element it names"""
    frm = next(i for i, it in enumerate(items) if it[1] == elem)
    c0 = r._alloc(1)
    r._push(wire.Op(cid, c0, "list_move", pos=to, move_from=frm, elem=elem))
    del items[frm]
    items.insert(to, ((r.peer, c0), elem))


def _raw_set(r, cid, elem, value):
    r._push(wire.Op(cid, r._alloc(1), "list_set", elem=elem, value=value))


def _raw_base(r, n):
    """`n` elements inserted by `r` as its first change (the row that n appends fuse into): items (peer, i), elements (peer, lamport i)"""
    assert r.next_counter == 0
    r._push(wire.Op(ML, r._alloc(n), "list_insert", pos=0, values=list(range(n)))); r.commit()
    return [((r.peer, i), (r.peer, i)) for i in range(n)]


def row_pass_docs():
    """k_mlist_post takes the rows of a change 64 at a time: ONE change of 63, 64, 65 and 129 move rows over distinct elements (a
    move row never fuses with its neighbour), a variant with a set row after every move, and for each a sibling document with the
    same rows one per change.  A second peer moves and sets some of the same elements concurrently, so the maxima are contested
    across the passes; the checkouts end inside the long change, on both sides of a pass boundary."""
    out = []
    for n in (63, 64, 65, 129):
        for sets in (False, True):
            for one_change in (True, False):
                a, b = wire.Replica(900 + n), wire.Replica(40 + n)
                items = _raw_base(a, n + 3)
                b.merge_from(a)
                theirs = list(items)
                first = a.next_counter
                for i in range(n):
                    _raw_move(a, ML, items, (a.peer, i), (i * 7 + 3) % (n + 3))
                    if sets:
                        _raw_set(a, ML, (a.peer, (i * 5) % (n + 3)), "s%d" % i)
                    if not one_change:
                        a.commit()
                a.commit()
                for i in range(0, n, 9):
                    _raw_move(b, ML, theirs, (a.peer, i), (i * 3) % (n + 3))
                    _raw_set(b, ML, (a.peer, (i * 5) % (n + 3)), "t%d" % i)
                b.commit()
                per = 2 if sets else 1
                snaps = [([(a.peer, first + k * per - 1)], None) for k in (1, 62, 63, 64, 65, 128) if k <= n]
                snaps += [([(a.peer, first + 64 * per - 1 if n >= 64 else first + 5), (b.peer, b.next_counter - 1)], None)]
                out.append(_all_versions("%d move rows%s, %s" % (n, " with sets" if sets else "", "one change" if one_change else "one per change"),
                                         [a, b], snaps))
    return out


def table_load_doc(n=1500):
    """About `n` elements inserted in bulk, then every one both moved and set once — two keys of the document's hash table per
    element, and a list of many leaves.  Two peers work concurrently on interleaved halves (and each on every 50th element of the
    other's, so some maxima are contested)."""
    a, b = wire.Replica(77), wire.Replica(33)
    items = _raw_base(a, n)
    b.merge_from(a)
    rng = random.Random(n)
    snaps = []
    for r, mine, half in ((a, items, 0), (b, list(items), 1)):
        for k, i in enumerate([i for i in range(n) if i % 2 == half or i % 50 == 7]):
            _raw_move(r, ML, mine, (a.peer, i), rng.randrange(n))
            _raw_set(r, ML, (a.peer, i), "%s%d" % ("ab"[half], i))
            if k % 100 == 99:
                r.commit()
                snaps.append(([(r.peer, r.next_counter - 1)], None))
        r.commit()
    d = Doc("%d elements, each moved and set" % n, [a, b], snaps, n_versions=3)
    assert len(d.model.value()["ml"]) == n
    return d


def split_maxima_docs():
    """(doc, {name: frontiers}): versions that hold an element's losing move but not its winner, a set but not the later set, the
    version just before and just after a set_container (the child appears, the plain value is gone), and a later plain set that
    replaces the child — the child's own ops, also later ones, must not show."""
    a, b = wire.Replica(60), wire.Replica(80)
    a.mlist_insert("ml", 0, ["a", "b", "c"]); a.commit()
    _sync([a, b])
    at = {}
    a.mlist_move("ml", 1, 0); a.commit(); at["losing move only"] = list(a.frontiers)              # b a c
    b.mlist_move("ml", 1, 2); b.commit(); at["winning move only"] = list(b.frontiers)             # a c b — the greater peer
    at["both moves"] = at["losing move only"] + at["winning move only"]
    _sync([a, b])
    a.mlist_set("ml", 2, "s1"); a.commit(); at["first set"] = list(a.frontiers)
    a.mlist_set("ml", 2, "s2"); a.commit(); at["second set"] = list(a.frontiers)
    child = a.mlist_set_container("ml", 2, wire.KIND_TEXT)
    at["before set_container"], at["at set_container"] = [(a.peer, child.counter - 1)], [(a.peer, child.counter)]
    a.text_insert(child, 0, "kid"); a.commit(); at["child written"] = list(a.frontiers)
    _sync([a, b])
    a.mlist_set("ml", 2, "plain"); a.commit(); at["plain set"] = list(a.frontiers)
    b.text_insert(child, 3, "s"); b.commit(); at["child written concurrently"] = list(b.frontiers)
    _sync([a, b])
    b.text_insert(child, 0, "late "); b.commit()        # an op on a child nothing refers to any more
    d = _all_versions("checkouts that split the maxima", [a, b], [(fr, None) for fr in at.values()])
    want = {"losing move only": ["b", "a", "c"], "winning move only": ["a", "c", "b"], "both moves": ["a", "c", "b"], "first set": ["a", "c", "s1"],
            "second set": ["a", "c", "s2"], "before set_container": ["a", "c", "s2"], "at set_container": ["a", "c", ""], "child written": ["a", "c", "kid"],
            "plain set": ["a", "c", "plain"], "child written concurrently": ["a", "c", "kids"], None: ["a", "c", "plain"]}
    return d, at, want


def children_docs():
    """(docs, values).  A child Text made by mlist_insert_container is written to by one peer while another moves its element
    concurrently: the child follows the element.  A child made by mlist_set_container competes with a concurrent plain set of the
    same lamport, both ways round by peer id."""
    docs, want = [], []
    a, b, c = wire.Replica(11), wire.Replica(5), wire.Replica(8)
    a.mlist_insert("ml", 0, ["a", "b", "c"])
    child = a.mlist_insert_container("ml", 1, wire.KIND_TEXT)
    a.text_insert(child, 0, "hello"); a.commit()
    _sync([a, b, c])
    a.text_insert(child, 5, " world"); a.commit()
    b.mlist_move("ml", 1, 3); b.text_insert(child, 0, ">"); b.commit()
    c.mlist_move("ml", 1, 0); c.commit()
    snaps = _ids_of(a, 1) + _ids_of(b) + _ids_of(c)
    _sync([a, b, c])
    docs.append(_all_versions("a child text follows its moved element", [a, b, c], snaps))
    want.append([">hello world", "a", "b", "c"])               # equal lamports: peer 8's move wins over peer 5's
    for pp, pq, child_wins in ((9, 6, True), (6, 9, False)):
        x, p, q = wire.Replica(7), wire.Replica(pp), wire.Replica(pq)
        x.mlist_insert("ml", 0, ["a", "b", "c"]); x.commit()
        _sync([x, p, q])
        child = p.mlist_set_container("ml", 1, wire.KIND_MAP)
        p.map_set(child, "k", 1); p.commit()
        q.mlist_set("ml", 1, "plain"); q.commit()
        snaps = [([(p.peer, 0)], None), ([(p.peer, 1)], None), ([(q.peer, 0)], None)]
        _sync([x, p, q])
        q.map_set(child, "late", 2); q.commit()
        docs.append(_all_versions("set_container against a plain set, the container's peer is the %s" % ("greater" if child_wins else "smaller"), [x, p, q], snaps))
        want.append(["a", {"k": 1, "late": 2} if child_wins else "plain", "c"])
    return docs, want
