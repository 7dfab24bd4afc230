"""Documents that arrive in steps (lm_stage + lm_import + lm_run, resident trackers) for the tests of the plain merge model's `Session`
(tests/_merge_ref.py): fuzz sessions whose writers take their view from the model, hand-built groups aimed at the places where a
stored tracker is continued or given up, and snapshot bases (lm_snapshot_base.h) as two-step sessions.  Shared by
tests/test_merge_ref_steps.py (oracle, kernel-logic harness) and tests/test_gpu_zz_merge_ref_steps.py.

Every hand-built GROUP knows its path: after every run `resident_fresh()` — the documents the integrate stage replayed from the empty
version — is asserted EXACTLY (`groups()`: one number per run; the first run replays every document).  Where the source names the
boundary the number comes from it; where it names none it was observed once on the kernel-logic harness and is asserted since,
harness and GPU alike.  What the source says (lm_k_integrate_span.h):
  * k_res_layout gives a peer first seen with extent e a region of ((e + e/2 + 64 + 31) & ~31) element slots; a peer that outgrows its
    region (`<=` in its region test) has the document LAID OUT ANEW.  A layout that moved costs a Text / List document nothing but its
    loc[] / kept[] words, which the integrate stage writes again from the stored leaves (:1723-1751) — its tracker CONTINUES,
    resident_fresh() stays 0.  Only a MovableList document loses its tracker with its layout (:1679-1687: a move keeps the id of the
    item it deleted in its element slot) and is replayed.  So the region-growth and new-peer groups are built twice: as Text (0 at
    capacity and at capacity + 1) and as MovableList (0 at capacity, the document count at capacity + 1).
  * "new peers that do not fit behind the old regions" (k_res_layout `top > rd.elem_cap` with `same`): the host sizes the slice for
    1.5 x atoms + 96 x (peers + 1) + 8 slots before it runs (lm_pipeline.h:1078), which bounds any fresh layout, and a stored region was
    sized from a smaller extent than the one it holds now — the branch cannot be reached while the host's rule stands.  What can be
    built is the step at which the host hands out a larger slice: the slice moves, tk[4..5] differ, the layout is anew (MovableList:
    replayed; Text: continued).
  * a new peer that sorts in front of a stored one renumbers the stored leaves (:1678, :1739-1746).  A Text / List document continues;
    a MovableList document is replayed (:1682-1685, since this module found that the ids its moves keep in cp[] were not renumbered:
    "movable list" and "new peers, ml" pin it).
  * other causes of a replay from the empty version, all on the host (lm_pipeline.h): the leaf pool outgrown (:1100-1104, capacity
    lc + lc/2 + 8 leaves), the tracker record outgrown (:1106 / tk_grow: more peers than P + P/2 + 2 or more containers than
    C + C/2 + 4 of the run that sized it), a failed run (:1619-1621), and in the kernel a stored directory beyond the optimistic one
    (:1766, the retry launch).  `Layout` restates all but the last two over the delivered changes.
Every number in `groups()` is written down as a literal AND is what `predicted_fresh` gives for the group's inputs; the harness showed
the same numbers when the groups were first run (the leaf-pool and record rules were added to `Layout` after it showed replays the
layout rule alone did not explain: 24 of 24 in the nested corpus, 17 of 19 predicted in the MovableList one, none unpredicted).

Fuzz sessions (step_corpora): four corpora — text / list / map with styles, text only, nested containers, MovableList — of documents
with at most 120 writer steps and 4 peers, cut into 5 - 6 steps by _resident.chunked_blobs / plan_steps, checked out only at versions
the step has applied (a five-step session ends with a step that brings nothing).  Every third flat / text session ends with a replica
that deletes all of the root Text and List, so that roots stay shown empty.  Sizes (SEEDS): the fewest seeds, in steps of ten, at
which check_step_conditions holds — for flat + text + nested together (10 / 10 / 30: what binds is diff_right_less, 54) and for the
MovableList corpus alone (110: winner_deleted_loser_alive, 11; 9 at 100)."""
import itertools, random

import _fuzz, _merge_docs, _merge_ref, _resident
from _richtext_ref import changes_of
from loro_amd import wire

V = _merge_ref.view
TEXT, ML = _merge_docs.TEXT, _merge_docs.ML


def part(changes):
    """one update blob of one peer's consecutive changes -> (blob, changes)"""
    changes = list(changes)
    return (wire.encode_updates(wire.split_blocks(changes)), changes)


def own(r, lo=0, hi=None):
    return r.changes.get(r.peer, [])[lo:hi]


class StepDoc:
    """one session: per step the blobs, the changes they hold, the checkout; and the model's result of every step"""

    def __init__(self, label, changes, steps):
        """steps: [([(blob, changes)], frontiers as a list of ids or None)]"""
        self.label, self.changes = label, list(changes)
        self.steps = [(list(parts), None if fr is None else list(fr)) for parts, fr in steps]
        self._model_steps()

    def _model_steps(self):
        s = _merge_ref.Session(self.changes)
        self.want, self.latest, self.pending_ids, self.sticky, self.overturned, self.later_loses = [], [], [], set(), 0, 0
        prev = None
        for parts, fr in self.steps:
            self.want.append(s.step([c for _, cs in parts for c in cs], fr))
            m = s.model
            self.latest.append(m.json(None, s.shown))
            ids = {(c.peer, k) for c in s.delivered for k in range(c.counter, c.ctr_end)}
            self.pending_ids.append(ids - m.all_ids)
            now = m.seen_roots() | (m.seen_roots(fr) if fr is not None else set())
            self.sticky |= {c for c in s.shown if c not in now}
            if prev is not None:
                a, b = _map_turns(prev, m)
                self.overturned += a; self.later_loses += b
            prev = m
        self.session = s

    def padded(self, n):
        """the same session with steps that bring nothing and render the latest version, up to `n` steps"""
        if len(self.steps) == n:
            return self
        return StepDoc(self.label, self.changes, self.steps + [([], None)] * (n - len(self.steps)))

    def wire_steps(self):
        return [([b for b, _ in parts], None if fr is None else wire.encode_frontiers(fr)) for parts, fr in self.steps]

    def extents(self):
        """per step: peer -> the gap-free extent of what was delivered of it (k_dag_a `covered`); peers only named by a dependency: 0"""
        out, have = [], {}
        for parts, _ in self.steps:
            for _, cs in parts:
                for c in cs:
                    have.setdefault(c.peer, []).append((c.counter, c.ctr_end))
                    for p, _k in c.deps:
                        have.setdefault(p, [])
            ext = {}
            for p, spans in have.items():
                e = 0
                for lo, hi in sorted(spans):
                    if lo <= e:
                        e = max(e, hi)
                ext[p] = e
            out.append(ext)
        return out


def _map_turns(prev, cur):
    """(overturned, later_loses) between two steps' models: per Map key that had a winner and received applied writes the winner's
    author had not seen — the winner changed to one of them / stayed"""
    a = b = 0
    for cid, keys in cur.maps.items():
        for key, entries in keys.items():
            if cid not in prev.maps or key not in prev.maps[cid]:
                continue
            old = prev.map_winner(cid, key, prev.all_ids)
            new = [e for e in entries if e[2] not in prev.all_ids and old[2] not in cur.closure_of_id(e[2])]
            if not new:
                continue
            win = cur.map_winner(cid, key, cur.all_ids)
            if win[2] != old[2]:
                a += any(e[2] == win[2] for e in new)
            else:
                b += 1
    return a, b


# ------------------------------------------------------------------------------------------------------------------- the layout rule
def region(e):
    """element slots of a peer first seen with extent `e` (k_res_layout)"""
    return (e + e // 2 + 64 + 31) & ~31


class Layout:
    """k_res_layout and the host's sizing of a resident document's slice, leaf pool and tracker record (lm_pipeline.h:1074-1106),
    restated over what was delivered.  step(ext, …) -> the set of reasons why the stored layout / tracker is given up, empty = continued:
    "region" / "slice" (the layout is anew), "record" / "leaves" (the tracker is not used)"""

    def __init__(self):
        self.cap, self.top, self.slice, self.pcap, self.ccap, self.leaves = {}, 0, 0, 0, 0, 0

    def step(self, ext, n_cont=0, n_el=0, n_op=0, n_nodes=0):
        why = set()
        atoms, P = sum(ext.values()), len(ext)
        need = atoms + atoms // 2 + 96 * (P + 1) + 8
        if need > self.slice:
            self.slice = ((need + need // 2 + 640) + 31) & ~31
            why.add("slice")
        lc = min(n_el // 32, (3 * n_op + 2 * n_nodes * P + 64) // 32) + 2 * n_cont + 2          # (span-granular leaves: resident documents always)
        if lc > self.leaves:
            self.leaves = lc + lc // 2 + 8
            why.add("leaves")
        if self.pcap == 0 or P > self.pcap or n_cont > self.ccap:
            self.pcap, self.ccap = P + P // 2 + 2, n_cont + n_cont // 2 + 4
            why.add("record")
        if any(ext.get(p, 0) > c for p, c in self.cap.items()):
            why.add("region")
        if not why & {"region", "slice"}:
            top = self.top + sum(region(ext[p]) for p in ext if p not in self.cap)
            if top > self.slice:
                why.add("slice")
        if why & {"region", "slice"}:
            self.cap, self.top = {}, 0
        for p in sorted(ext):
            if p not in self.cap:
                self.cap[p] = region(ext[p]); self.top += self.cap[p]
        return why


INSERTS = ("text_insert", "list_insert", "style_start", "style_end", "list_move")


def step_reasons(doc):
    """per step: the reasons `Layout` gives, from the changes delivered up to it — containers that an op addresses, op rows, the
    elements its insert rows make, DAG nodes (k_dag_a: an applied change whose only dependency is its peer's previous op continues
    the node of the change in front of it)"""
    lay, out = Layout(), []
    conts, delivered, n_el, n_op = set(), [], 0, 0
    for (parts, _), ext in zip(doc.steps, doc.extents()):
        for _, cs in parts:
            for c in cs:
                delivered.append(c)
                for o in c.ops:
                    conts.add(o.cid)
                    n_op += 1
                    if o.kind in INSERTS:
                        n_el += o.atom_len
        end = _merge_ref.applied_ends(delivered)
        applied = sorted({(c.peer, c.counter): c for c in delivered if c.ctr_end <= end.get(c.peer, 0)}.values(), key=lambda c: (c.peer, c.counter))
        nodes = sum(1 for i, c in enumerate(applied) if not (i and applied[i - 1].peer == c.peer and c.counter > 0 and list(c.deps) == [(c.peer, c.counter - 1)]))
        out.append(lay.step(ext, len(conts), n_el, n_op, nodes))
    return out


def is_movable(doc):
    return any(o.cid.kind == wire.KIND_MOVABLE for c in doc.changes for o in c.ops)


def predicted_anew(doc):
    """per step >= 1: does the restatement say that a region or the slice is outgrown (the layout is anew)?"""
    return [bool(w & {"region", "slice"}) for w in step_reasons(doc)[1:]]


def predicted_fresh(doc):
    """per step >= 1: does the restatement say that the stored tracker is not used?  The record or the leaf pool is outgrown
    (lm_pipeline.h:1100-1106); a MovableList document also when its layout is anew or its peers are renumbered
    (lm_k_integrate_span.h:1678-1687)"""
    ml = is_movable(doc)
    return [bool(w & {"record", "leaves"}) or (ml and (bool(w) or rn)) for w, rn in zip(step_reasons(doc)[1:], renumbered(doc))]


def renumbered(doc):
    """per step >= 1: does the step bring a peer that sorts in front of a stored one?  (The stored leaves are renumbered,
    lm_k_integrate_span.h:1678; a MovableList document is replayed instead: the ids its moves keep in cp[] are not reached.)"""
    ext = doc.extents()
    return [any(p < q for p in ext[k] if p not in ext[k - 1] for q in ext[k - 1]) for k in range(1, len(ext))]


def ml_fresh(docs):
    """resident_fresh() after every run of MovableList documents: the layout moved or the peers were renumbered"""
    per = [predicted_fresh(d) for d in docs]
    return [len(docs)] + [sum(x[k] for x in per) for k in range(len(per[0]))]


# ------------------------------------------------------------------------------------------------------------------- fuzz sessions
def _chunked(reps, rng, max_chunk=4):
    """_resident.chunked_blobs together with the changes each blob holds (the same random stream: replayed beside it)"""
    twin = random.Random(); twin.setstate(rng.getstate())
    blobs = _resident.chunked_blobs(reps, rng, max_chunk)
    out = []
    for r in reps:
        chs, i = own(r), 0
        while i < len(chs):
            k = twin.randint(1, max_chunk)
            out.append((blobs[len(out)], chs[i:i + k])); i += k
    assert len(out) == len(blobs)
    return out


def fuzz_session(label, reps, versions, rng, n_steps, n_pad=6):
    parts = _chunked(reps, rng)
    plan = _resident.plan_steps(parts, rng, n_steps)               # (no checkouts yet: picked below among what the step has applied)
    steps, delivered = [], []
    for ps, _ in plan:
        delivered += [c for _, cs in ps for c in cs]
        fr = None
        if versions and rng.random() < 0.4:
            end = _merge_ref.applied_ends(delivered)
            ok = [v for v in versions if all(end.get(p, 0) > k for p, k in v)]
            if ok:
                fr = rng.choice(ok)
        steps.append((ps, fr))
    return StepDoc(label, changes_of(reps), steps).padded(n_pad)


def _empty_the_roots(reps):
    """the last replica takes everything in and deletes all of the root Text and List: their states stay (sticky), shown empty"""
    r = reps[-1]
    for o in reps[:-1]:
        r.merge_from(o)
    for cid in (TEXT, wire.root_cid("list", wire.KIND_LIST)):
        if cid in r.seq:
            r.set_visible(cid.name, cid.kind, V(r, cid))
            if r.seq[cid]:
                (r.text_delete if cid.kind == wire.KIND_TEXT else r.list_delete)(cid.name, 0, len(r.seq[cid]))
    r.commit()


def step_corpora(n_seeds=None):
    """name -> [StepDoc]"""
    n = n_seeds or SEEDS
    out = {"flat": [], "text": [], "nested": [], "movable": []}
    for name in out:
        for seed in range(n[name]):
            rng = random.Random(seed * 7 + 1)
            snaps = []
            if name == "flat":
                reps = _fuzz.random_session(1000 + seed, n_peers=rng.randint(2, 4), n_steps=rng.randint(60, 120), kinds=("text", "list", "map"), snapshots=snaps, styles=True, max_del=[4, 30][seed % 2], view=V)
            elif name == "text":
                reps = _fuzz.random_session(2000 + seed, n_peers=rng.randint(2, 4), n_steps=rng.randint(80, 120), kinds=("text",), snapshots=snaps, styles=seed % 2 == 0, max_ins=8, max_del=[4, 4, 30][seed % 3], view=V)
            elif name == "nested":
                reps = _fuzz.nested_session(3000 + seed, n_peers=3, n_steps=120, view=V)
                snaps = [([(r.peer, ch.ctr_end - 1)], None) for r in reps for ch in own(r)[1::4]]
            else:
                reps = _fuzz.movable_session(4000 + seed, n_peers=3 + seed % 2, n_steps=120, nested=seed % 2 == 0, snapshots=snaps, view=V)
            if name in ("flat", "text") and seed % 3 == 0:
                _empty_the_roots(reps)
            versions = [list(fr) for fr, _ in snaps]
            cuts =_merge_docs.delete_run_cuts(_merge_ref.Model(changes_of(reps)))
            out[name].append(fuzz_session("%s seed %d" % (name, seed), reps, versions + cuts[:3], rng, 5 + seed % 2))
    return out


SEEDS = {"flat": 10, "text": 10, "nested": 30, "movable": 110}
CONDITIONS = {"pending_steps": 20, "resolving_steps": 20, "checkouts_that_differ": 20, "sticky_roots": 10, "overturned": 20, "later_loses": 20}


def step_counts(docs):
    tot = dict.fromkeys(_merge_ref.OUTCOMES + tuple(CONDITIONS), 0)
    for d in docs:
        for k, v in d.session.model.cross.items():
            tot[k] += v
        for k in range(len(d.steps)):
            tot["pending_steps"] += bool(d.pending_ids[k])
            tot["resolving_steps"] += k > 0 and bool(d.pending_ids[k - 1] - d.pending_ids[k])
            tot["checkouts_that_differ"] += d.steps[k][1] is not None and d.want[k][1] != d.latest[k]
        tot["sticky_roots"] += len(d.sticky)
        tot["overturned"] += d.overturned
        tot["later_loses"] += d.later_loses
    return tot


def check_step_conditions(corpora):
    """asserted from the model and the inputs alone, before anything is compared.  The flat, text and nested corpora together, and the
    MovableList corpus alone (whose root is shown at every version and whose Map is small: no sticky roots, no Map turns asked of it)"""
    plain = step_counts([d for k, ds in corpora.items() if k != "movable" for d in ds])
    mv = step_counts(corpora["movable"])
    for name, tot in (("flat + text + nested", plain), ("movable", mv)):
        for k in _merge_ref.OUTCOMES:
            assert tot[k] >= (1 if k == "diff_right_equal" else 50), (name, k, tot)
        for k, least in CONDITIONS.items():
            assert tot[k] >= least or (name == "movable" and k in ("sticky_roots", "overturned", "later_loses")), (name, k, tot)
    el = _merge_docs.outcome_counts([_Final(d) for d in corpora["movable"]])
    for k, least in _merge_docs.MOVABLE_AT_LEAST.items():
        assert el[k] >= least, (k, el)
    for ds in corpora.values():
        for d in ds:
            assert len(d.steps) == 6 and len({c.peer for c in d.changes}) <= 4, d.label
    return plain, mv


class _Final:
    def __init__(self, d):
        self.model = d.session.model


# ---------------------------------------------------------------------------------------------------------------- hand-built groups
def peer_steps(label, reps, order, first=None, fronts=None):
    """step 0: `first` (changes of one peer; default: nothing special), then one step per replica of `order` with the rest of its own
    changes.  `fronts`: step -> checkout"""
    fronts = fronts or {}
    steps = []
    if first:
        steps.append(([part(first)], fronts.get(0)))
    skip = {(c.peer, c.counter) for c in first or ()}
    for r in order:
        rest = [c for c in own(r) if (c.peer, c.counter) not in skip]
        steps.append(([part(rest)] if rest else [], fronts.get(len(steps))))
    return StepDoc(label, changes_of(reps), steps)


def region_growth_docs(kind):
    """(docs at capacity, docs at capacity + 1): one peer first seen with e atoms grows in ONE later step to its region's capacity / one
    past it, then by one atom more.  `kind`: "text" or "ml"."""
    at, past = [], []
    for e in (1, 31, 32, 33, 1000):
        for extra, out in ((0, at), (1, past)):
            r = wire.Replica(100 + e)
            target = region(e) + extra

            def grow(n):
                if kind == "text":
                    r.text_insert("text", len(r.seq.get(TEXT, [])), "".join(chr(97 + i % 26) for i in range(n)))
                else:
                    r.mlist_insert("ml", r.mlist_len("ml"), list(range(n)))
                r.commit()
            grow(e); grow(target - e); grow(1)
            chs = own(r)
            assert [c.ctr_end for c in chs] == [e, target, target + 1]
            behind = wire.Replica(1 << 40)            # a second peer whose region lies behind: a new layout moves it
            _writer(kind, behind, 3, "B")
            steps = [([part(chs[:1]), part(own(behind))], None), ([part(chs[1:2])], None), ([part(chs[2:])] if extra else [], None)]
            d = StepDoc("%s: %d atoms, then %d (capacity %d)" % (kind, e, target, region(e)), chs[:3 if extra else 2] + own(behind), steps)
            want = [bool(w) for w in predicted_anew(d)]
            assert want == [bool(extra), False], (d.label, want)
            out.append(d)
    return at, past


EDGE = [7, (1 << 32) - 1, (1 << 32) + 5, (1 << 63) - 1, (1 << 63) + 5, (1 << 64) - 1]


def _writer(kind, r, n, tag):
    if kind == "text":
        r.text_insert("text", 0, (tag * n)[:n])
    else:
        r.mlist_insert("ml", 0, ["%s%d" % (tag, i) for i in range(n)])
    r.commit()


def new_peer_docs(kind):
    """stored peers 2^32 + 5 and 2^63 + 5; then one step each for a peer that sorts before all stored ones, between them, after them
    — for every choice of the three among ids on both sides of 2^32 and 2^63.  Concurrent writers: nothing waits."""
    docs = []
    for before, between, after in ((7, (1 << 63) - 1, (1 << 64) - 1), ((1 << 32) - 1, (1 << 32) + 6, (1 << 63) + 6), (1, 1 << 33, 1 << 63 | 1 << 32)):
        for order in itertools.permutations((before, between, after)):
            reps = [wire.Replica(p) for p in ((1 << 32) + 5, (1 << 63) + 5) + order]
            for i, r in enumerate(reps):
                _writer(kind, r, 3 + i, "pqrst"[i])
            steps = [([part(own(reps[0])), part(own(reps[1]))], None)] + [([part(own(r))], None) for r in reps[2:]]
            docs.append(StepDoc("%s: new peers %s" % (kind, list(order)), changes_of(reps), steps))
    return docs


def lane_trip_docs(kind):
    """63 peers stored; 64, 65, 66 after one step each (the layout loops take 64 peers per trip); the new peer sorts first / in the
    middle / last"""
    docs = []
    for where in (0, 1, 2):
        rng = random.Random(63 + where)
        ids = sorted(rng.sample(range(1 << 20, 1 << 62), 66))
        late = [ids[0], ids[1], ids[2]] if where == 0 else [ids[30], ids[31], ids[32]] if where == 1 else [ids[63], ids[64], ids[65]]
        reps = {p: wire.Replica(p) for p in ids}
        for i, p in enumerate(ids):
            _writer(kind, reps[p], 1 + i % 3, "abcdefgh"[i % 8])
        steps = [([part(own(reps[p])) for p in ids if p not in late], None)] + [([part(own(reps[p]))], None) for p in late]
        docs.append(StepDoc("%s: 63 peers, then three more %s" % (kind, ("in front", "in the middle", "behind")[where]), changes_of(reps.values()), steps))
    return docs


def slice_growth_docs(kind):
    """a peer of 1,000 atoms resident (slice of 3,200 slots); a step brings two new peers of 700 atoms each, both sorting behind it:
    1.5 x 2,400 + 96 x 4 + 8 > 3,200 — the host hands out a larger slice, the layout is anew; then one atom more (continues).  (Three
    peers fit the tracker record sized for one, P + P/2 + 2.)"""
    a = wire.Replica(5000)
    _writer(kind, a, 1000, "a")
    others = [wire.Replica(p) for p in (5001, 5002)]
    for i, r in enumerate(others):
        _writer(kind, r, 700, "bc"[i])
    _writer(kind, a, 1, "z")
    d = StepDoc("%s: two new peers outgrow the slice" % kind, changes_of([a] + others),
                [([part(own(a, 0, 1))], None), ([part(own(r)) for r in others], None), ([part(own(a, 1))], None)])
    assert predicted_anew(d) == [True, False]
    return [d]


def pending_docs():
    """(rendered at the latest version throughout, with a checkout in the middle step).  B and C continue A's text; their changes are
    delivered first and wait (tk[7] != 0 after that run: DF_FILL_KEPT must stay off in the next), then A's base resolves them, then an
    ordinary step."""
    out = ([], [])
    for s in range(4):
        rng = random.Random(40 + s)
        a, b, c = wire.Replica(300 + s), wire.Replica(200 + s), wire.Replica(400 + s)
        a.text_insert("text", 0, "".join(chr(97 + i % 26) for i in range(20 + 30 * s))); a.commit()
        a.text_delete("text", 3, 4); a.commit()
        mid = list(a.frontiers)
        _merge_docs._sync([a, b, c])
        for r, t in ((b, "B"), (c, "C")):
            for k in range(3 + s):
                n = len(r.seq[TEXT])
                r.text_insert("text", rng.randint(0, n), t * rng.randint(1, 3))
                r.text_delete("text", rng.randrange(n - 2), 2)
                r.commit()
        x = wire.Replica(900 + s); x.map_set("map", "k", s); x.list_insert("list", 0, [s]); x.commit()      # applies at once
        _merge_docs._sync([a, b, c])
        a.text_insert("text", 0, "tail"); a.commit()
        n0 = 2
        for k, fr in enumerate((None, mid)):
            steps = [([part(own(b)), part(own(x))], None), ([part(own(a, 0, n0)), part(own(c))], fr), ([part(own(a, n0))], None)]
            d = StepDoc("pending across steps %d%s" % (s, ", checked out in the middle" if fr else ""), changes_of([a, b, c, x]), steps)
            assert d.want[0][3] > 0 and d.want[1][3] == 0 and d.pending_ids[0] and not d.pending_ids[1]
            out[k].append(d)
    return out


def checkout_docs():
    """no new blobs: a change end, inside a delete run, a two-peer frontier, [], back to the latest version; then an import while the
    document is checked out, and a last return"""
    docs = []
    for d0 in _merge_docs.backspace_docs()[:4] + _merge_docs.id_window_docs()[:2]:
        reps = d0.reps
        m = d0.model
        a, b = reps[0], reps[1]
        last = {r.peer: own(r)[-1] for r in reps}
        held = [c for r in reps for c in own(r)[:-1]]
        end = _merge_ref.applied_ends(held)
        cuts = [v for v in _merge_docs.delete_run_cuts(m) if end[v[0][0]] > v[0][1]]
        cut = cuts[len(cuts) // 2]
        ch = own(a)[len(own(a)) // 2]
        two = sorted([(a.peer, own(a)[1].ctr_end - 1), (b.peer, own(b)[0].ctr_end - 1)])
        assert all(end[p] > k for p, k in [cut[0]] + two)
        steps = [([part(own(r)[:-1]) for r in reps], None), ([], [(ch.peer, ch.ctr_end - 1)]), ([], cut), ([], two), ([], []), ([], None), ([], cut),
                 ([part([last[r.peer]]) for r in reps], None), ([], two), ([], None)]
        docs.append(StepDoc("checkouts of %s" % d0.label, changes_of(reps), steps))
    return docs


def three_peer_docs():
    """(peer by peer in all six orders, change by change).  three_peer_text(70 / 130 / 300): concurrent inserts in every leaf's first and
    last slot against a resident tail that is one leaf, three leaves, more than LM_DIR_OPT_MAX=4 allows"""
    by_peer, by_run = [], []
    for n in (70, 130, 300):
        d0 = _merge_docs.three_peer_text(n, n)
        for order in itertools.permutations(d0.reps):
            by_peer.append(peer_steps("%s, delivered %s" % (d0.label, [d0.reps.index(r) for r in order]), d0.reps, order))
        chs = sorted(changes_of(d0.reps), key=lambda c: (c.lamport, c.peer))
        by_run.append(StepDoc("%s, change by change" % d0.label, chs, [([part([c])], None) for c in chs]))
    n = max(len(d.steps) for d in by_run)
    return by_peer, [d.padded(n) for d in by_run]


def _prefix_and_branches(reps):
    """a document that begins as one chain: (the chain's changes, [the rest of every peer])"""
    p0 = min((c for r in reps for c in own(r)), key=lambda c: (c.lamport, c.peer)).peer
    base = []
    for c in next(own(r) for r in reps if r.peer == p0):
        if any(p != p0 for p, _ in c.deps):
            break
        base.append(c)
    heads = [k for r in reps if r.peer != p0 for c in own(r) for p, k in c.deps if p == p0]
    if heads:                                                   # the chain ends where the first other peer took it over
        base = [c for c in base if c.ctr_end - 1 <= min(heads)]
    skip = {(c.peer, c.counter) for c in base}
    return base, [[c for c in own(r) if (c.peer, c.counter) not in skip] for r in reps]


def branch_docs(docs):
    """the base resident, every branch a step of its own, in both orders"""
    out = []
    for d0 in docs:
        base, branches = _prefix_and_branches(d0.reps)
        branches = [b for b in branches if b]
        for rev in (False, True):
            steps = [([part(base)], None)] + [([part(b)], None) for b in (branches[::-1] if rev else branches)]
            out.append(StepDoc("%s, branches %s" % (d0.label, "reversed" if rev else "in order"), changes_of(d0.reps), steps).padded(4))
    return out


def window_docs():
    """one peer's run is resident up to a counter of 15 / 16 / 17 / 31 / 32 / 33 (the 16-id window of loc[], the 32-slot word of kept[]
    and of tk[6]); the next step brings the rest of the run and the first half of the concurrent deletes and inserts across the
    16-aligned counters, the last one the other half"""
    out = []
    for s, cut in enumerate((15, 16, 17, 31, 32, 33)):
        for name, make in (("id windows", id_window_reps), ("backspace", backspace_reps)):
            reps = make(s, cut)
            first = own(reps[0])[0]
            assert first.counter == 0 and first.ctr_end == cut, (name, cut, first.ctr_end)
            rest = sorted([c for c in changes_of(reps) if c is not first], key=lambda c: (c.lamport, c.peer))
            halves = [rest[:len(rest) // 2], rest[len(rest) // 2:]]
            steps = [([part([first])], None)]
            for h in halves:
                steps.append(([part([c for c in h if c.peer == p]) for p in sorted({c.peer for c in h})], None))
            d = StepDoc("%s, resident up to counter %d" % (name, cut), changes_of(reps), steps)
            assert not any(d.pending_ids)
            out.append(d)
    return out


def id_window_reps(s, cut):
    """_merge_docs.id_window_docs, the long run committed in two changes: [0, cut) and the rest"""
    rng = random.Random(900 + s)
    a, b, c = wire.Replica(50 + s), wire.Replica(20 + s), wire.Replica(90 + s)
    run = "".join(chr(97 + i % 26) for i in range(100))
    a.text_insert("text", 0, run[:cut]); a.commit()
    a.text_insert("text", cut, run[cut:]); a.commit()
    _merge_docs._sync([a, b, c])
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
        _merge_docs._sync([a, b, c])
    return [a, b, c]


def backspace_reps(s, cut):
    """_merge_docs.backspace_docs over a base committed in two changes, every backspace / delete run placed around counter 16 or 32"""
    rng = random.Random(1200 + s)
    reps = [wire.Replica(p) for p in rng.sample(range(1, 1 << 20), 3)]
    run = "".join(chr(97 + i % 26) for i in range(60))
    reps[0].text_insert("text", 0, run[:cut]); reps[0].commit()
    reps[0].text_insert("text", cut, run[cut:]); reps[0].commit()
    _merge_docs._sync(reps)
    for rnd in range(2):
        for r in reps:
            n = len(r.seq[TEXT])
            k = rng.randint(2, 6)
            pos = min(n - k - 1, max(k, rng.choice((16, 32)) + rng.randint(-1, 2)))
            r.commit()
            if rng.random() < 0.6:
                for j in range(k):
                    r.text_delete("text", pos - j, 1)
            else:
                for j in range(k):
                    r.text_delete("text", pos, 1)
            r.text_insert("text", rng.randint(0, len(r.seq[TEXT])), "XY"[:rng.randint(1, 2)])
            r.commit()
        _merge_docs._sync(reps)
    return reps


def movable_docs():
    """lamport_tie_docs, move_against_delete_docs and split_maxima_docs: the list's first change resident, then every competitor's
    moves / sets in a step of its own, in both orders"""
    out = []
    src = [d for d in _merge_docs.lamport_tie_docs() if "reverse" not in d.label] + _merge_docs.move_against_delete_docs()[0] + [_merge_docs.split_maxima_docs()[0]]
    for d0 in src:
        maker = d0.reps[0]
        for rev in (False, True):
            order = d0.reps[::-1] if rev else d0.reps
            out.append(peer_steps("%s, %s" % (d0.label, "reversed" if rev else "in order"), d0.reps, order, first=own(maker, 0, 1)).padded(5))
    return out


def map_docs():
    """Lamport ties between the edge peer ids with the two writes in different steps, in both orders; a child Map hidden by a write
    delivered later (and earlier); a delete that wins, delivered first (and last)"""
    out = []
    E = _merge_docs_map_edge_peers()
    for p, q in itertools.combinations(E, 2):
        for first, second in ((p, q), (q, p)):
            a, b = wire.Replica(first), wire.Replica(second)
            for r in (a, b):
                r.map_set("m", "k", "from %d" % r.peer); r.map_set("m", "k%d" % (r.peer % 3), r.peer % 1000); r.commit()
            d = StepDoc("a tie between %d (first) and %d" % (first, second), changes_of([a, b]), [([part(own(a))], None), ([part(own(b))], None), ([], [(first, 0)])])
            assert d.session.model.value()["m"]["k"] == "from %d" % max(p, q) and d.overturned + d.later_loses >= 1
            out.append(d)
    for pc, ps in ((9, 6), (6, 9)):
        x, p, q = wire.Replica(7), wire.Replica(pc), wire.Replica(ps)
        x.map_set("m", "k", 0); x.commit()
        _merge_docs._sync([x, p, q])
        child = p.map_set_container("m", "k", wire.KIND_MAP)
        p.map_set(child, "in", 1); p.commit()
        q.map_set("m", "k", "plain"); q.commit()
        _merge_docs._sync([x, p, q])
        q.map_set(child, "late", 2); q.commit()
        for order in ((p, q), (q, p)):
            out.append(peer_steps("a child Map (peer %d) against a scalar (peer %d), %d first" % (pc, ps, order[0].peer), [x, p, q], order, first=own(x)))
    for first in (0, 1):
        a, b = wire.Replica(50), wire.Replica(40)
        a.map_set("m", "k", "set"); a.commit()
        b.map_set("m", "other", 1); b.map_delete("m", "k"); b.commit()
        order = (b, a) if first == 0 else (a, b)
        d = StepDoc("a delete that wins, delivered %s" % ("first" if first == 0 else "last"), changes_of([a, b]), [([part(own(r))], None) for r in order] + [([], None)])
        assert d.session.model.value() == {"m": {"other": 1}}
        out.append(d)
    return out


def _merge_docs_map_edge_peers():
    import _merge_docs_map
    return _merge_docs_map.EDGE_PEERS


def groups():
    """[(name, environment, [StepDoc], resident_fresh() after every run or None where a count per run is derived by the caller)]"""
    out = []
    for kind in ("text", "ml"):
        at, past = region_growth_docs(kind)
        out.append(("region growth to capacity, " + kind, {}, at, [5, 0, 0]))                                       # src: `<=` in the region test
        out.append(("region growth past capacity, " + kind, {}, past, [5, 0, 0] if kind == "text" else [5, 5, 0]))  # src: :1679-1683
        docs = new_peer_docs(kind)
        out.append(("new peers, " + kind, {}, docs, [len(docs), 0, 0, 0] if kind == "text" else ml_fresh(docs)))     # src: a new peer's region lies behind the old ones;
        docs = lane_trip_docs(kind)                                                                                  # a MovableList is replayed when it sorts in front (:1678-1686)
        out.append(("63 to 66 peers, " + kind, {}, docs, [3, 0, 0, 0] if kind == "text" else [3, 2, 2, 2]))
        assert kind == "text" or ml_fresh(docs) == [3, 2, 2, 2]
        out.append(("slice outgrown, " + kind, {}, slice_growth_docs(kind), [1, 0, 0] if kind == "text" else [1, 1, 0]))
    latest, checked = pending_docs()
    out.append(("pending across steps", {}, latest, [4, 0, 0]))
    out.append(("pending across steps, checked out", {}, checked, [4, 0, 0]))
    out.append(("checkouts with no new blobs", {}, checkout_docs(), [6] + [0] * 9))
    by_peer, by_run = three_peer_docs()
    out.append(("three peers, peer by peer", {}, by_peer, [18, 4, 8]))                        # (the leaf pool is outgrown: lm_pipeline.h:1100-1104)
    run_fresh = [3] + [0] * 32
    run_fresh[3], run_fresh[8], run_fresh[28] = 2, 2, 1
    out.append(("three peers, change by change", {}, by_run, run_fresh))
    out.append(("three peers, peer by peer, LM_DIR_OPT_MAX=4", {"LM_DIR_OPT_MAX": "4"}, by_peer, [18, 4, 8]))
    docs = branch_docs(_merge_docs.sweep_docs())
    out.append(("leaf sweep, branch by branch", {}, docs, [len(docs), 0, 0, 0]))
    out.append(("linear prefix, branch by branch", {}, branch_docs(_merge_docs.linear_prefix_docs()), [12, 0, 0, 0]))
    out.append(("loc[] / kept[] windows", {}, window_docs(), [12, 0, 0]))
    out.append(("movable list", {}, movable_docs(), [38, 9, 25, 12, 0]))                     # (a competitor that sorts in front of the stored peers: replayed)
    out.append(("map", {}, map_docs(), [36, 0, 0]))
    for name, _, docs, fresh in out:          # every number above is also what the restated rules give for these inputs
        per = [predicted_fresh(d) for d in docs]
        assert fresh == [len(docs)] + [sum(x[k] for x in per) for k in range(len(per[0]))], name
    return out


# ---------------------------------------------------------------------------------------------------------------------- running
def oracle_column(doc, upto):
    """what the oracle's Session says at step `upto` (the third column of a failure message)"""
    import _oracle
    o = _oracle.Session()
    try:
        for blobs, fr in doc.wire_steps()[:upto + 1]:
            got = o.step(blobs, fr)
    finally:
        o.close()
    return got


def run_group(ctx, name, docs, fresh=None, what="kernel"):
    """the sessions of `docs` (equally many steps each) on `ctx` — a harness Context or the device's MergeEngine: lm_stage + lm_import
    for the first step, lm_import for the others; every result of every step against the model's, resident_fresh() after every run
    against `fresh` exactly.  -> the counts seen"""
    n = len(docs[0].steps)
    assert all(len(d.steps) == n for d in docs), name
    ws = [d.wire_steps() for d in docs]
    seen = []
    for k in range(n):
        blobs, fr = [w[k][0] for w in ws], [w[k][1] for w in ws]
        if k == 0:
            ctx.stage(blobs, fr)
            ctx.import_more([[] for _ in docs], fr)          # resident from the first run on
        else:
            ctx.import_more(blobs, fr)
        ctx.run()
        got = ctx.fetch()
        seen.append(ctx.resident_fresh())
        assert len(got) == len(docs)
        for d, g in zip(docs, got):
            if g != d.want[k]:
                raise AssertionError("%s, %s, step %d at %s:\n %s %r\n model  %r\n oracle %r" % (name, d.label, k, d.steps[k][1], what, g, d.want[k], oracle_column(d, k)))
        if fresh is not None:
            assert seen == fresh[:k + 1], "%s: resident_fresh() after every run %r, expected %r" % (name, seen, fresh)
    return seen


# ------------------------------------------------------------------------------------------------------------------ snapshot bases
class BaseDoc:
    """[snapshot of the history up to a critical version, the updates beyond it] (lm_snapshot_base.h).  The snapshot's state section is
    written by the oracle's state writer (_oracle.state_entries); the EXPECTED values are the model's: the session stands at the base
    version and then takes the updates.  `batch`: the document as one import_batch; `steps`: the snapshot first, then one step per
    peer's updates."""

    def __init__(self, label, reps, base, taken=True, **snap_kw):
        import _oracle
        p0 = base[0].peer
        assert all(c.peer == p0 for c in base) and base[0].counter == 0
        early = wire.Replica(p0)
        early.changes = {p0: list(base)}; early.vv = {p0: base[-1].ctr_end}; early.frontiers = [(p0, base[-1].ctr_end - 1)]
        st, ents = _oracle.state_entries([early.export()])
        assert st in (0, 4), st
        snap = early.export_snapshot(state=ents, **snap_kw)
        skip = {(c.peer, c.counter) for c in base}
        rest = [[c for c in own(r) if (c.peer, c.counter) not in skip] for r in reps]
        rest = [part(cs) for cs in rest if cs]
        self.label, self.taken = label, taken                      # taken: rebase_updates_on_state accepts the document
        self.many_pieces = False                                   # more deletes of base content than LM_PD_STATE_PIECES=0 leaves room for
        self.batch = [snap] + [b for b, _ in rest]
        changes = changes_of(reps)
        two = StepDoc(label, changes, [([(snap, base)], None), (rest, None)])
        self.want = two.want[1]
        self.steps = StepDoc(label + ", peer by peer", changes, [([(snap, base)], None)] + [([p], None) for p in rest])
        self.deletes_base = any(o.kind == "delete" and o.del_id[0] == p0 and o.del_id[1] < base[-1].ctr_end for c in changes if (c.peer, c.counter) not in skip for o in c.ops)


def base_corpus(seeds=range(700, 730)):
    """state_base_docs of tests/test_emu_snapshot.py with the writers' views from the model: a solo prefix handed to concurrent branches"""
    out = []
    for seed in seeds:
        rng = random.Random(seed)
        reps = _fuzz.random_session(seed, n_peers=rng.randint(2, 3), n_steps=rng.randint(30, 90), kinds=("text", "list", "map"), solo_steps=rng.randint(10, 60), max_ins=10, view=V)
        p0 = reps[0].peer
        heads = [d[1] for r in reps[1:] for c in own(r)[:1] for d in c.deps if d[0] == p0]
        if not heads:
            continue
        base = [c for c in own(reps[0]) if c.ctr_end <= min(heads) + 1]
        if not base or base[-1].ctr_end != min(heads) + 1:
            continue
        out.append(BaseDoc("base seed %d" % seed, reps, base, **([dict(), dict(block_size=256)][seed % 2])))
    return out


def _base(text="abcdefghij", peers=(41, 42), text_only=False):
    reps = [wire.Replica(p) for p in peers]
    a = reps[0]
    a.text_insert("t", 0, text)
    if not text_only:
        a.list_insert("l", 0, [1, 2, 3, 4, 5, 6]); a.map_set("m", "k", "base")
    a.commit()
    base = own(a)
    _merge_docs._sync(reps)
    return reps, base


def base_hand_docs():
    T = wire.root_cid("t", wire.KIND_TEXT)
    out = []
    (a, b), base = _base(text_only=True)
    a.text_insert("t", 10, "XYZ"); a.commit()
    a.text_delete("t", 8, 4); a.commit()                                   # (41, 8) (41, 9) of the base and two of the run above it, ids contiguous
    assert [o.kind for o in own(a)[-1].ops] == ["delete"] and own(a)[-1].ops[0].del_id == (41, 8)
    b.text_insert("t", 9, "b"); b.commit()
    out.append(BaseDoc("a delete run partly below and partly above the base", [a, b], base))
    (a, b), base = _base()
    for j in range(4):
        a.text_delete("t", 6 - j, 1)
    a.commit()
    assert own(a)[-1].ops[0].signed_len == -4
    b.text_insert("t", 5, "in"); b.text_delete("t", 0, 2); b.commit()
    out.append(BaseDoc("a reversed span over base content", [a, b], base))
    (a, b), base = _base()
    a.text_delete("t", 2, 3); a.list_delete("l", 1, 2); a.commit()
    b.text_delete("t", 3, 3); b.list_delete("l", 2, 2); b.commit()
    _merge_docs._sync([a, b])
    a.text_insert("t", 2, "|"); a.commit()
    out.append(BaseDoc("the same base elements deleted by two concurrent branches", [a, b], base))
    (a, b), base = _base()
    a.text_delete("t", 1, 6); a.list_delete("l", 0, 5); a.commit()
    b.text_insert("t", 4, "kept"); b.list_insert("l", 3, ["kept"]); b.commit()
    out.append(BaseDoc("a base range deleted concurrently with an insert inside it", [a, b], base))
    (a, b, c), base = _base(peers=(41, 42, 40))
    for r, ch in ((a, "A"), (b, "B"), (c, "C")):
        r.text_insert("t", 10, ch * 2); r.text_insert("t", 4, ch); r.text_insert("t", 0, ch * 3); r.list_insert("l", 0, [ch]); r.list_insert("l", 7, [ch + "end"]); r.commit()
    out.append(BaseDoc("concurrent inserts at position 0, at the end and at one gap", [a, b, c], base))
    a, b = wire.Replica(41), wire.Replica(42)
    a.text_insert("t", 0, "hello world"); cm = a.map_set_container("m", "child", wire.KIND_MAP); a.map_set(cm, "x", 1)
    ct = a.map_set_container("m", "note", wire.KIND_TEXT); a.text_insert(ct, 0, "abc")
    cl = a.list_insert_container("l", 0, wire.KIND_LIST); a.list_insert(cl, 0, [1, 2, 3]); a.commit()
    base = own(a)
    _merge_docs._sync([a, b])
    a.map_set(cm, "y", "new"); a.text_insert(ct, 3, "DEF"); a.list_insert(cl, 1, ["mid"]); a.map_set(cm, "x", 3); a.commit()
    b.text_insert(ct, 0, "<"); b.map_set(cm, "x", 2); b.list_delete(cl, 0, 2); b.list_insert(cl, 1, ["b"]); b.commit()
    out.append(BaseDoc("base child Map / Text / List edited by two concurrent updates", [a, b], base))
    assert out[-1].want[1] == b'{"l":[["mid",3,"b"]],"m":{"child":{"x":3,"y":"new"},"note":"<abcDEF"},"t":"hello world"}', out[-1].want[1]
    # more by-position pieces than the 64 a document gets under LM_PD_STATE_PIECES=0 (lm_pipeline.h:1195, PD_CAP + 1): the list
    # overflows and the document is replayed from the snapshot's history (redo_documents)
    (a, b), base = _base(text="".join(chr(97 + i % 26) for i in range(400)))
    for i in range(90):
        a.text_delete("t", i + 1, 1)                                        # every other base character: no two targets are neighbours
    a.commit()
    for i in range(30):
        b.text_insert("t", 13 * i, "B")
    b.text_delete("t", 200, 40); b.commit()
    out.append(BaseDoc("ninety scattered deletes of base content", [a, b], base))
    out[-1].many_pieces = True
    # declined: B has seen only the first of the base's two changes
    a, b = wire.Replica(41), wire.Replica(42)
    a.text_insert("t", 0, "first"); a.commit()
    _merge_docs._sync([a, b])
    a.text_insert("t", 5, " second"); a.commit()
    base = own(a)
    b.text_insert("t", 0, "B:"); b.text_delete("t", 3, 2); b.commit()
    out.append(BaseDoc("an update concurrent with part of the base", [a, b], base, taken=False))
    return out
