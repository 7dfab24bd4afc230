"""Import mode and common ancestors of every step of a resident document (k_import_lca, lm_import_modes / lm_import_lca): the
expectation and the documents, shared by tests/test_import_lca.py (oracle, kernel-logic harness) and tests/test_gpu_zz_import_lca.py.

What a step must answer is stated over SETS OF IDS from the plain model (tests/_merge_ref.py: `Model(changes, delivered=…)`,
`closure_of_id`); no node, span, heap or oracle code is used for it.  F is the applied set before the step, T the applied set after it
(pending changes are in neither; a failed step delivers nothing).  heads(S) = the last id of every peer of S that lies in the closure
of no other peer's last id.  For a reported (mode, L):
  S0  T == F  =>  (Linear, heads(F)) exactly (diff_calc.rs:150-152): an empty step, a step that only adds pending changes, a
      duplicate blob, a checkout-only step.
  S1  every id of L lies in F.
  S2  the ids of L are pairwise causally incomparable and sorted by (peer id as u64, counter) in the encoded bytes.
  S3  mode ImportGreaterUpdates or Linear  =>  L == heads(F) (and F <= T, which holds for every import): what dag.rs:993-1008
      literally asserts.  The stronger reading of diff_calc.rs:91-102 — "every change of T \\ F has all of F in its causal past" — is
      NOT kept by the reference: with F = {7@0..4, 9@0} and a step that brings 7@5..7, written without knowledge of 9@0, the walk
      trims B's span of peer 7 to A's head (dag.rs:698-703), both heads come out Shared and the mode is ImportGreaterUpdates ("two
      failed steps in a row", step 4).  ImportGreaterUpdates says that T contains F, not that nothing new is concurrent to F.
  S4  mode Linear  =>  additionally the ids of T \\ F form one causal chain.
  S5  the mode is never Checkout for a step that grew the version (oplog.rs:610-615); it is None only for a failed step and where
      a hand-built document pins it (more than 16 common ancestors, more than 64 heads: the kernel's header comment).
S1-S3 are the reference's own property test (dag.rs:966-1009) plus the DiffMode contract.  They hold for the ORACLE's answers on all
of the corpus and the hand-built groups (test_import_lca.py asserts it first), so the contract is not misread.

Exact answers: the restatement at the end of this module (dag.rs:487-765 over plain node tuples, written from the reference's text,
checked against the known answers of dag.rs:1108-1276 without the oracle) over the REFERENCE's node partition — has_succ and splits
simulated in delivery order, pending changes entering when they apply (`Delivered`, run beside the model) — gives the expected
(mode, L) of every step (`expected`).  Every hand-built document also carries its answers as LITERALS (`LcaDoc.want`): written by
hand from dag.rs for the "after a failure" group, read off the oracle once for the others (so not independent of it) and each checked
against S0-S5 and the restatement.  Node partitions: never cut (the oracle), cut at successors (k_dag_a under LM_CUT_MIN_ROWS=0) and
as delivered agree on all 1,081 steps, and the starts of the delivered nodes lie between the other two's
(test_import_lca.py::test_partitions_agree); with every change a node of its own, a partition nobody builds, 5 steps differ.

Corpus (`corpus()`): 140 fuzz sessions of the existing writers with their view from the model, six steps each; every fifth session has
one blob damaged (last byte flipped: checksum mismatch, status 2) at a random step and all blobs of that step delivered again with
the next one.  Counts over corpus + hand-built groups (187 documents, 1,081 steps that go through), from the model and the restatement,
never from the oracle or the code under test; floors in FLOORS, asserted before any comparison:
  Linear 609, Import 323, ImportGreaterUpdates 149; L with >= 2 ids 207; from with >= 2 heads 390; grows right after a failed step 33;
  leaves pending 439, resolves pending 257; brings a peer sorting in front of a stored one 144; T == F 449."""
import random

import _fuzz, _merge_ref, _resident
from _merge_docs_steps import part, _chunked
from _richtext_ref import changes_of
from loro_amd import wire

V = _merge_ref.view
N_STEPS = 6
FLOORS = {"Linear": 50, "Import": 50, "ImportGreaterUpdates": 50, "lca_two_or_more": 20, "from_two_or_more_heads": 20,
          "grows_after_failed": 20, "leaves_pending": 20, "resolves_pending": 20, "peer_in_front": 20, "unchanged": 20}
UNKNOWN = (None, None)


def decode_frontiers(b):
    """Frontiers::encode() bytes -> [(peer, counter)] in the encoded order"""
    def uleb(i):
        v = s = 0
        while True:
            x = b[i]; i += 1
            v |= (x & 0x7F) << s; s += 7
            if not x & 0x80:
                return v, i
    n, i = uleb(0)
    out = []
    for _ in range(n):
        p, i = uleb(i)
        z, i = uleb(i)
        out.append((p, (z >> 1) ^ -(z & 1)))
    assert i == len(b), "bytes behind the frontiers"
    return out


def damaged(blob):
    b = bytearray(blob); b[-1] ^= 1
    return bytes(b)


class Fact:
    """what the model knows about one step"""
    __slots__ = ("failed", "model", "F", "T", "heads_F", "grew", "new_pending", "resolved", "peer_in_front", "after_failed", "nodes")


class Delivered:
    """the reference's DAG nodes as a session builds them (oplog/loro_dag.rs:302-367 handle_new_change, :547-597
    handle_deps_break_points, :945-968 slice; no lazy loading: every node is in memory).  A change that depends on nothing but its
    peer's previous atom extends that peer's last node unless the node `has_succ`; any other change is a node of its own, and every
    dependency of it on ANOTHER peer marks the node it ends (`has_succ`) or splits the node it falls inside — the front keeps its
    flag, the tail depends on the front's last atom and inherits the flag.  Changes enter in delivery order: the step's blobs in
    order, the changes of a blob by counter, pending changes in their delivery order as soon as they apply (the least fixpoint of
    _merge_ref.applied_ends, run in that order)."""

    def __init__(self):
        self.nodes = {}          # peer -> [[counter, atoms, lamport, deps, has_succ]] by counter
        self.end = {}
        self.waiting = []

    def _node_at(self, p, c):
        for i, n in enumerate(self.nodes.get(p, ())):
            if n[0] <= c < n[0] + n[1]:
                return i, n
        raise KeyError((p, c))

    def _apply(self, p, counter, ctr_end, lamport, deps):
        ns = self.nodes.setdefault(p, [])
        if len(deps) == 1 and deps[0][0] == p and ns and not ns[-1][4]:
            last = ns[-1]
            assert last[0] + last[1] == counter and last[2] + last[1] == lamport and deps[0][1] == counter - 1
            last[1] += ctr_end - counter
        else:
            ns.append([counter, ctr_end - counter, lamport, [tuple(d) for d in deps], False])
            for q, k in deps:
                if q == p:
                    continue
                i, t = self._node_at(q, k)
                if t[0] + t[1] - 1 == k:
                    t[4] = True
                else:
                    cut = k - t[0] + 1
                    self.nodes[q].insert(i + 1, [t[0] + cut, t[1] - cut, t[2] + cut, [(q, k)], t[4]])
                    t[1] = cut
        self.end[p] = ctr_end

    def deliver(self, changes):
        self.waiting += list(changes)
        progress = True
        while progress:
            progress, rest = False, []
            for c in self.waiting:
                have = self.end.get(c.peer, 0)
                if c.ctr_end <= have:
                    continue
                if c.counter <= have and all(self.end.get(p, 0) > k for p, k in c.deps):
                    if c.counter == have:
                        self._apply(c.peer, c.counter, c.ctr_end, c.lamport, list(c.deps))
                    else:      # (a change that overlaps the applied end: its tail applies, on top of the peer's last atom)
                        self._apply(c.peer, have, c.ctr_end, c.lamport + have - c.counter, [(c.peer, have - 1)])
                    progress = True
                else:
                    rest.append(c)
            self.waiting = rest

    def snapshot(self):
        return [(p, n[0], n[1], n[2], list(n[3])) for p, ns in self.nodes.items() for n in ns]


def heads(m, S):
    last = {}
    for p, c in S:
        last[p] = max(last.get(p, -1), c)
    ids = sorted(last.items())
    cl = {i: m.closure_of_id(i) for i in ids}
    return [i for i in ids if not any(i in cl[o] for o in ids if o != i)]


class LcaDoc:
    """one session.  steps: [([(blob, changes)], frontiers as a list of ids / None, fails)] — `fails`: the step carries a damaged
    blob and the engine drops all of it.  `want`: per step the literal (mode, [ids]) or UNKNOWN; `status`: per step the literal status.
    `oracle_differs`: steps where the kernel's pinned answer is UNKNOWN by its own limits and the oracle knows more."""

    def __init__(self, label, changes, steps, want=None, status=None, oracle_differs=(), no_oracle_from=N_STEPS):
        self.label, self.changes = label, list(changes)
        steps = [(list(s[0]), s[1], bool(s[2]) if len(s) > 2 else False) for s in steps]
        self.steps = steps + [([], None, False)] * (N_STEPS - len(steps))
        assert len(self.steps) == N_STEPS, label
        self.want, self.status, self.oracle_differs = want, status, set(oracle_differs)
        self.no_oracle_from = no_oracle_from   # from this step on the engine refuses what the oracle takes (an engine limit)
        self._facts = None

    def wire_steps(self):
        return [([b for b, _ in parts], None if fr is None else wire.encode_frontiers(fr)) for parts, fr, _ in self.steps]

    def facts(self):
        if self._facts is None:
            out, delivered, F, pend, prev_failed, m, dag = [], [], frozenset(), frozenset(), False, None, Delivered()
            for parts, _, fails in self.steps:
                f = Fact()
                f.failed, f.after_failed = fails, prev_failed
                prev_failed = fails
                if fails:
                    out.append(f)
                    continue
                now = [c for _, cs in parts for c in cs]
                if now or m is None:
                    delivered += now
                    m = _merge_ref.Model(self.changes, delivered=delivered)
                dag.deliver(now)
                f.model, f.F, f.T, f.nodes = m, F, m.all_ids, dag.snapshot()
                assert {(n[0], k) for n in f.nodes for k in range(n[1], n[1] + n[2])} == f.T, "the delivered DAG is the model's applied set"
                assert F <= f.T
                f.heads_F = heads(m, F)
                f.grew = f.T != F
                p_now = frozenset((c.peer, k) for c in delivered for k in range(c.counter, c.ctr_end)) - f.T
                f.new_pending, f.resolved = bool(p_now - pend), bool(pend - p_now)
                old_peers = {p for p, _ in F}
                f.peer_in_front = bool(old_peers) and any(p not in old_peers and p < max(old_peers) for p, _ in f.T - F)
                F, pend = f.T, p_now
                out.append(f)
            self._facts = out
        return self._facts


def check_answer(f, info, where=""):
    """S0-S5 for one step that did not fail; `info` = (mode name, encoded frontiers)"""
    mode, enc = info
    assert mode is not None and enc is not None, (where, "S5: no answer", info)
    L = decode_frontiers(enc)
    m = f.model
    if not f.grew:
        assert (mode, L) == ("Linear", f.heads_F), (where, "S0", mode, L, f.heads_F)
    for i in L:
        assert i in f.F, (where, "S1", i)
    assert L == sorted(L), (where, "S2: order", L)
    for a in L:
        for b in L:
            assert a == b or a not in m.closure_of_id(b), (where, "S2: comparable", a, b)
    new = f.T - f.F
    if mode in ("ImportGreaterUpdates", "Linear"):
        assert L == f.heads_F, (where, "S3: L", mode, L, f.heads_F)
    if mode == "Linear" and new:
        chain = sorted(new, key=lambda i: len(m.closure_of_id(i)))
        for a, b in zip(chain, chain[1:]):
            assert a in m.closure_of_id(b), (where, "S4", a, b)
    assert not (f.grew and mode == "Checkout"), (where, "S5: Checkout for an import that grew the version")


def expected(d):
    """per step the exact (mode, L) from the restatement (below) over the reference's partition, simulated in delivery order
    (`Delivered`); test_import_lca.py::test_partitions_agree holds the other two partitions against it"""
    if getattr(d, "_expected", None) is None:
        d._expected = [None if f.failed else restated(f, as_delivered) for f in d.facts()]
    return d._expected


def counts(docs, modes_of):
    """the FLOORS quantities; `modes_of(doc)` -> per step (mode, encoded L) from a reference that is not the code under test"""
    tot = dict.fromkeys(FLOORS, 0)
    for d in docs:
        ref = modes_of(d)
        for f, r in zip(d.facts(), ref):
            if f.failed:
                continue
            if r is None:
                continue
            if r[0] in tot:
                tot[r[0]] += 1
            tot["lca_two_or_more"] += r[1] is not None and len(decode_frontiers(r[1])) >= 2
            tot["from_two_or_more_heads"] += len(f.heads_F) >= 2
            tot["grows_after_failed"] += f.after_failed and f.grew
            tot["leaves_pending"] += f.new_pending
            tot["resolves_pending"] += f.resolved
            tot["peer_in_front"] += f.peer_in_front
            tot["unchanged"] += not f.grew
    return tot


# ----------------------------------------------------------------------------------------------------------------------- running
def run(make_ctx, docs):
    """every step of every document as ONE batch -> per step [(status, info)] per document"""
    sessions = [d.wire_steps() for d in docs]
    out = []
    with make_ctx() as c:
        for k in range(N_STEPS):
            blobs = [s[k][0] for s in sessions]
            fr = [s[k][1] for s in sessions]
            if k == 0:
                c.stage(blobs, fr); c.import_more([[] for _ in blobs], fr)
            else:
                c.import_more(blobs, fr)
            c.run()
            got, info = c.fetch(), c.import_info()
            out.append([(g, i) for g, i in zip(got, info)])
    return out


def api_edges(make_ctx):
    """before any resident run: -1; a folded batch: -1 for all; `cap` one byte short: -1"""
    import ctypes
    a = wire.Replica(7); a.text_insert("text", 0, "hello"); a.commit()
    blob = a.export()
    v = wire.encode_frontiers([(7, 2)])
    with make_ctx() as c:
        c.stage([[blob], [blob], [blob]], [v, None, v])
        assert c.b.shared_documents(c.h) > 0
        assert c.import_info() == [UNKNOWN] * 3                  # folded, and no resident run yet
        c.run()
        assert c.import_info() == [UNKNOWN] * 3
        c.import_more([[], [], []], [v, None, v])
        assert c.b.shared_documents(c.h) == 0
        assert c.import_info() == [("Linear", wire.encode_frontiers([]))] * 3   # lm_import ran the staged blobs as the first step
        c.run()
        want = wire.encode_frontiers([(7, 4)])
        assert c.import_info() == [("Linear", want)] * 3
        buf = ctypes.create_string_buffer(64)
        assert c.b.import_lca(c.h, 1, buf, len(want)) == len(want) and buf.raw[:len(want)] == want
        assert c.b.import_lca(c.h, 1, buf, len(want) - 1) == -1
        assert c.b.import_lca(c.h, 3, buf, 64) == -1               # no such document


def oracle_run(docs):
    """the same from the oracle's Session: per step [(result, info or UNKNOWN for a step that failed)] per document"""
    import _oracle
    out = [[] for _ in range(N_STEPS)]
    for d in docs:
        o = _oracle.Session()
        for k, (blobs, fr) in enumerate(d.wire_steps()):
            w = o.step(blobs, fr)
            out[k].append((w, o.import_info() if w[0] in (0, 4, 6) else UNKNOWN))
        o.close()
    return out


def check_run(docs, got, oracle=None, what="kernel"):
    """`got` = run(...) of the code under test: S0-S5 from the model, the literals of the hand-built documents, the statuses, and —
    where `oracle` (oracle_run of the same documents) is given — results and answers step by step as _import_info_matches does"""
    for i, d in enumerate(docs):
        for k, f in enumerate(d.facts()):
            (res, info) = got[k][i]
            where = "%s: %s, step %d" % (what, d.label, k)
            if d.status is not None:
                assert res[0] == d.status[k], (where, "status", res[0], d.status[k])
            if f.failed:
                assert res[0] != 0 and info == UNKNOWN, (where, "a failed step answers nothing", res[0], info)
                if oracle is not None and k < d.no_oracle_from:
                    assert res == oracle[k][i][0], (where, "result", str(res)[:200], str(oracle[k][i][0])[:200])
                continue
            if d.want is not None:
                w = d.want[k]
                shown = UNKNOWN if info == UNKNOWN else (info[0], decode_frontiers(info[1]))
                assert shown == w, (where, "literal", shown, w)
            if d.want is None or d.want[k] != UNKNOWN:
                check_answer(f, info, where)
                exact = expected(d)[k]
                assert (info[0], decode_frontiers(info[1])) == exact, (where, "restatement", info[0], decode_frontiers(info[1]), exact)
            if oracle is not None and k < d.no_oracle_from:
                ores, oinfo = oracle[k][i]
                assert res == ores, (where, "result", str(res)[:200], str(ores)[:200])
                if k not in d.oracle_differs:
                    assert info == oinfo, (where, "oracle", info, oinfo)


# ----------------------------------------------------------------------------------------------------------------------- writers
def _w(r, n=1):
    """one change of `n` atoms in the replica's own Text container (its own view is all it needs)"""
    name = "t%d" % r.peer
    r.text_insert(name, len(r.seq.get(wire.root_cid(name, wire.KIND_TEXT), ())), "abcdefghij"[:n])
    r.commit()
    return r.changes[r.peer][-1]


def _m(r):
    """one change of one atom in the shared Map (documents with many peers: one container)"""
    r.map_set("m", "k%d" % r.peer, r.next_counter)
    r.commit()
    return r.changes[r.peer][-1]


def _all(reps):
    seen, out = set(), []
    for r in reps:
        for chs in r.changes.values():
            for c in chs:
                if (c.peer, c.counter) not in seen:
                    seen.add((c.peer, c.counter)); out.append(c)
    return out


def _p(*changes):
    """one blob per run of changes of one peer"""
    out, run_ = [], []
    for c in changes:
        if run_ and (c.peer != run_[-1].peer or c.counter != run_[-1].ctr_end):
            out.append(part(run_)); run_ = []
        run_.append(c)
    if run_:
        out.append(part(run_))
    return out


def _bad(parts):
    return [(damaged(b), cs) for b, cs in parts]


# ----------------------------------------------------------------------------------------------------------------------- hand-built
def after_a_failure():
    """a step that fails leaves the document at the version of its last step that went through: the next step is measured from there"""
    docs = []
    a = wire.Replica(7); a1 = _w(a, 5); a2 = _w(a, 3); a3 = _w(a, 2)
    b = wire.Replica(9); b1 = _w(b, 1)
    ch = _all([a, b])
    L, I = "Linear", "Import"
    # peer 7 writes "hello"; peer 9's blob arrives damaged, then good: concurrent with peer 7 (was: ImportGreaterUpdates, [])
    docs.append(LcaDoc("failed, then a concurrent peer", ch, [(_p(a1), None), (_bad(_p(b1)), None, True), (_p(b1), None)],
                       want=[(L, []), UNKNOWN, (I, []), (L, [(7, 4), (9, 0)]), (L, [(7, 4), (9, 0)]), (L, [(7, 4), (9, 0)])], status=[0, 2, 0, 0, 0, 0]))
    # … peer 7 continues its own chain after the failed step (was: Linear, [])
    docs.append(LcaDoc("failed, then the own chain", ch, [(_p(a1), None), (_bad(_p(a2)), None, True), (_p(a2), None), (_p(a3), None)],
                       want=[(L, []), UNKNOWN, (L, [(7, 4)]), (L, [(7, 7)]), (L, [(7, 9)]), (L, [(7, 9)])], status=[0, 2, 0, 0, 0, 0]))
    docs.append(LcaDoc("the same without the failed step", ch, [(_p(a1), None), ([], None), (_p(b1), None)],
                       want=[(L, []), (L, [(7, 4)]), (I, []), (L, [(7, 4), (9, 0)]), (L, [(7, 4), (9, 0)]), (L, [(7, 4), (9, 0)])], status=[0] * 6))
    docs.append(LcaDoc("failed, then a checkout only", ch, [(_p(a1, a2), None), (_bad(_p(a3)), None, True), ([], [(7, 4)]), ([], None), (_p(a3), [(7, 7)])],
                       want=[(L, []), UNKNOWN, (L, [(7, 7)]), (L, [(7, 7)]), (L, [(7, 7)]), (L, [(7, 9)])], status=[0, 2, 0, 0, 0, 0]))
    docs.append(LcaDoc("two failed steps in a row", ch, [(_p(a1), None), (_bad(_p(a2)), None, True), (_bad(_p(b1)), None, True), (_p(b1), None), (_p(a2), None)],
                       want=[(L, []), UNKNOWN, UNKNOWN, (I, []), ("ImportGreaterUpdates", [(7, 4), (9, 0)]), (L, [(7, 7), (9, 0)])], status=[0, 2, 2, 0, 0, 0]))
    docs.append(LcaDoc("failed at step 0", ch, [(_bad(_p(a1)), None, True), (_p(a1), None), (_p(a2), None), (_bad(_p(a3)), None, True), (_p(b1), None)],
                       want=[UNKNOWN, (L, []), (L, [(7, 4)]), UNKNOWN, (I, []), (L, [(7, 7), (9, 0)])], status=[2, 0, 0, 2, 0, 0]))
    docs.append(LcaDoc("nothing went through yet: two failures, then two heads", ch, [(_bad(_p(a1)), None, True), (_bad(_p(b1)), None, True), (_p(a1, b1), None)],
                       want=[UNKNOWN, UNKNOWN, ("ImportGreaterUpdates", []), (L, [(7, 4), (9, 0)]), (L, [(7, 4), (9, 0)]), (L, [(7, 4), (9, 0)])], status=[2, 2, 0, 0, 0, 0]))
    # a refused checkout (status 6) between two imports: the import stands, the next `from` includes it
    docs.append(LcaDoc("refused checkout between two imports", ch, [(_p(a1), None), (_p(a2), [(99, 0)]), (_p(a3), None), (_p(b1), [(99, 0)]), ([], None)],
                       want=[(L, []), (L, [(7, 4)]), (L, [(7, 7)]), (I, []), (L, [(7, 9), (9, 0)]), (L, [(7, 9), (9, 0)])], status=[0, 6, 0, 6, 0, 0]))
    # a step that went through with a status of its own directly in front of a failed step, then growth: the host's "failed" test
    # (status != OK at the end of the run), the kept copy's and the kernel's must mean the same documents
    docs.append(LcaDoc("refused checkout, failed, growth", ch, [(_p(a1), None), (_p(a2), [(99, 0)]), (_bad(_p(a3)), None, True), (_p(a3), None), (_p(b1), None)],
                       want=[(L, []), (L, [(7, 4)]), UNKNOWN, (L, [(7, 7)]), (I, []), (L, [(7, 9), (9, 0)])], status=[0, 6, 2, 0, 0, 0]))
    # LM_UNSUPPORTED, soft: a Counter child under the Map is rendered as null and the document is flagged (4) at every step
    s_ = wire.Replica(7)
    s_.map_set_container("m", "c", wire.KIND_COUNTER); s_.map_set("m", "k", 1); s_.commit()
    s1 = s_.changes[7][-1]; s2 = _w(s_, 3); s3 = _w(s_, 2)
    t_ = wire.Replica(9); t1 = _w(t_, 1)
    docs.append(LcaDoc("unsupported (soft), failed, growth", _all([s_, t_]), [(_p(s1), None), (_bad(_p(s2)), None, True), (_p(s2), None), (_p(t1), None), (_p(s3), None)],
                       want=[(L, []), UNKNOWN, (L, [(7, 1)]), (I, []), ("ImportGreaterUpdates", [(7, 4), (9, 0)]), (L, [(7, 6), (9, 0)])], status=[4, 2, 4, 4, 4, 4]))
    return docs


def fast_exits():
    docs = []
    L, G = "Linear", "ImportGreaterUpdates"
    a = wire.Replica(1); a1 = _w(a, 1); a2 = _w(a, 1); a3 = _w(a, 3); a4 = _w(a, 2)
    docs.append(LcaDoc("empty to one chain", _all([a]), [(_p(a1, a2, a3), None), (_p(a4), None)],
                       want=[(L, []), (L, [(1, 4)]), (L, [(1, 6)]), (L, [(1, 6)]), (L, [(1, 6)]), (L, [(1, 6)])]))
    docs.append(LcaDoc("same peer, same node: counters 0, 1, last", _all([a]), [(_p(a1), None), (_p(a2), None), (_p(a3), None), (_p(a4), None)],
                       want=[(L, []), (L, [(1, 0)]), (L, [(1, 1)]), (L, [(1, 4)]), (L, [(1, 6)]), (L, [(1, 6)])]))
    docs.append(LcaDoc("a chain whose first change is missing", _all([a]), [(_p(a2, a3), None), ([], None), (_p(a1), None), (_p(a4), None)],
                       want=[(L, []), (L, []), (L, []), (L, [(1, 4)]), (L, [(1, 6)]), (L, [(1, 6)])]))
    a = wire.Replica(1); b = wire.Replica(2)
    a1 = _w(a, 2); b1 = _w(b, 2); a.merge_from(b); a2 = _w(a, 1); a3 = _w(a, 1)
    ch = _all([a, b])
    docs.append(LcaDoc("empty to one head above a merge node", ch, [(_p(a1, a2, b1), None), (_p(a3), None)],
                       want=[(G, []), (L, [(1, 2)]), (L, [(1, 3)]), (L, [(1, 3)]), (L, [(1, 3)]), (L, [(1, 3)])]))
    docs.append(LcaDoc("empty to two heads", ch, [(_p(a1, b1), None), (_p(a2), None), (_p(a3), None)],
                       want=[(G, []), (G, [(1, 1), (2, 1)]), (L, [(1, 2)]), (L, [(1, 3)]), (L, [(1, 3)]), (L, [(1, 3)])]))
    # same peer across a node boundary: peer 2 depends on (1, 0), peer 1 goes on from its own change, then on top of peer 2
    a = wire.Replica(1); b = wire.Replica(2)
    a1 = _w(a, 1); b.merge_from(a); b1 = _w(b, 1); a2 = _w(a, 2); a.merge_from(b); a3 = _w(a, 1); a4 = _w(a, 1)
    ch = _all([a, b])
    docs.append(LcaDoc("same peer across a node boundary", ch, [(_p(a1), None), (_p(a2), None), (_p(b1), None), (_p(a3), None), (_p(a4), None)],
                       want=[(L, []), (L, [(1, 0)]), ("Import", []), (G, [(1, 2), (2, 0)]), (L, [(1, 3)]), (L, [(1, 4)])]))
    docs.append(LcaDoc("a direct cross-peer dependency", ch, [(_p(a1), None), (_p(b1), None), (_p(a2), None), (_p(a3, a4), None)],
                       want=[(L, []), (G, [(1, 0)]), ("Import", []), (G, [(1, 2), (2, 0)]), (L, [(1, 4)]), (L, [(1, 4)])]))
    return docs


def branches():
    """a branch from the first, a middle and the last change of a resident run of n changes, then the merge change on both heads"""
    docs = []
    for n in (1, 2, 63, 64, 65):
        for cut in sorted({1, (n + 1) // 2, n}):
            a = wire.Replica(11); b = wire.Replica(5 if cut % 2 else 12)
            run_ = [_w(a, 2) for _ in range(cut)]
            b.merge_from(a); b1 = _w(b, 3)
            run_ += [_w(a, 2) for _ in range(n - cut)]
            a.merge_from(b); top = _w(a, 1)
            last = (11, 2 * n - 1)
            both = sorted([last, (b.peer, 2)])
            if cut == n:
                # (a change on top of another peer's: the walk pushes its dependency — not Linear any more, dag.rs:716-722 — and, one
                # step later, reaches peer 11's own previous op on B's side only: unmatched, the empty version, dag.rs:687-691)
                want = [("Linear", []), ("ImportGreaterUpdates", [last]), ("Import", [])]
            else:
                want = [("Linear", []), ("Import", []), ("ImportGreaterUpdates", both)]
            want += [("Linear", [(11, 2 * n)])] * 3
            docs.append(LcaDoc("branch at change %d of %d" % (cut, n), _all([a, b]), [(_p(*run_), None), (_p(b1), None), (_p(top), None)], want=want))
    return docs


def many_heads():
    """k heads and the change that merges all of them: 16 common ancestors are answered, 17 and more are not (LCA_MAXF), more than 64
    heads on either side are not (LCA_FMAX).  Step 0: k - 1 concurrent peers, step 1: one more (T has k heads: a concurrent step),
    step 2: the merge change."""
    docs = []
    for k in (2, 3, 15, 16, 17, 63, 64, 65):
        reps = [wire.Replica(100 + 3 * i) for i in range(k)]
        first = [_m(r) for r in reps]
        top = wire.Replica(50)
        for r in reps:
            top.merge_from(r)
        t = _m(top)
        hs = [(r.peer, 0) for r in reps]
        G = "ImportGreaterUpdates"
        want = [("Linear", []) if k == 2 else (G, []) if k - 1 <= 64 else UNKNOWN,
                ("Import", []) if k <= 64 else UNKNOWN,
                (G, hs) if k <= 16 else UNKNOWN] + [("Linear", [(50, 0)])] * 3
        diff = [s for s in range(3) if want[s] == UNKNOWN]
        docs.append(LcaDoc("%d heads" % k, _all(reps + [top]), [(_p(*first[:-1]), None), (_p(first[-1]), None), (_p(t), None)], want=want, oracle_differs=diff))
    return docs


def peers_between_steps():
    docs = []
    L = "Linear"
    ids = [(1 << 32) + 5, (1 << 63) + 5, 7, (1 << 32) + 9, (1 << 63) - 1, (1 << 64) - 1]
    # every step brings a new peer that has seen everything: in front of, between and behind the stored ones, around 2^32 and 2^63
    reps, chs = [], []
    for p in ids:
        r = wire.Replica(p)
        for o in reps:
            r.merge_from(o)
        chs.append(_w(r, 2)); reps.append(r)
    docs.append(LcaDoc("new peers, each on top of the last", _all(reps), [(_p(c), None) for c in chs],
                       want=[(L, [])] + [("ImportGreaterUpdates", [(ids[i - 1], 1)]) for i in range(1, 6)]))
    # … the same peers concurrent to each other
    reps = [wire.Replica(p) for p in ids]
    chs = [_w(r, 2) for r in reps]
    docs.append(LcaDoc("new peers, all concurrent", _all(reps), [(_p(c), None) for c in chs], want=[(L, [])] + [("Import", [])] * 5))
    # three-way lamport ties in the heap between peer ids on both sides of 2^32 and 2^63, in both delivery orders; then the merge
    for name, order in (("ascending", (0, 1, 2)), ("descending", (2, 1, 0)), ("middle last", (0, 2, 1))):
        tri = [wire.Replica(p) for p in (5, (1 << 32) + 5, (1 << 63) + 5)]
        base = wire.Replica(3); b0 = _w(base, 1)
        for r in tri:
            r.merge_from(base)
        one = [_w(r, 2) for r in tri]
        two = [_w(r, 2) for r in tri]
        top = wire.Replica(1 << 40)
        for r in tri:
            top.merge_from(r)
        t = _w(top, 1)
        o = order
        hs = sorted((tri[i].peer, 3) for i in range(3))
        docs.append(LcaDoc("lamport ties, " + name, _all(tri + [base, top]),
                           [(_p(b0, one[o[0]], two[o[0]]), None), (_p(one[o[1]], two[o[1]]), None), (_p(one[o[2]]), None), (_p(two[o[2]]), None), (_p(t), None)],
                           want=[(L, []), ("Import", []), ("Import", []), ("ImportGreaterUpdates", sorted([(tri[o[0]].peer, 3), (tri[o[1]].peer, 3), (tri[o[2]].peer, 1)])),
                                 ("ImportGreaterUpdates", hs), (L, [(1 << 40, 0)])]))
    return docs


def peer_counts():
    """63 -> 66 peers and 255 / 256 / 257 peers in one chain (every peer on top of the one before, ids in a shuffled order).  A
    document of more than MAX_PEERS - 1 = 255 peers is LM_UNSUPPORTED (4) from k_doc_tables on and answers nothing: the kernel's own
    `P > MAX_PEERS` test is never reached."""
    docs = []
    for n0, more in ((63, (1, 1, 1)), (254, (1, 1, 1))):
        rng = random.Random(n0)
        ids = rng.sample(range(1000, 1 << 20), n0 + sum(more))
        reps, chs = [], []
        for p in ids:
            r = wire.Replica(p)
            if reps:
                r.merge_from(reps[-1])
            chs.append(_m(r)); reps.append(r)
        steps = [(_p(*chs[:n0]), None)]
        at = n0
        for k in more:
            steps.append((_p(*chs[at:at + k]), None)); at += k
        want = [("Linear", [])] + [("ImportGreaterUpdates", [(ids[n0 - 1 + i], 0)]) for i in range(3)] + [("Linear", [(ids[-1], 0)])] * 2
        status = [0] * 6
        failing = []
        if n0 == 254:   # the 256th peer is refused (k_doc_tables: at most MAX_PEERS - 1 = 255 peers), and so is the 257th, whose
            # blob names the 256th as a dependency: the document stays at 255 peers
            want[2] = want[3] = UNKNOWN; want[4] = want[5] = ("Linear", [(ids[254], 0)]); status[2] = status[3] = 4; failing = [2, 3]
        steps = [(s[0], s[1], i in failing) for i, s in enumerate(steps)]
        docs.append(LcaDoc("%d peers, then %d" % (n0, n0 + 3), _all(reps), steps, want=want, status=status, no_oracle_from=2 if failing else N_STEPS))
    return docs


def large():
    """one document of more than LM_CUT_MIN_ROWS = 2,048 op rows: two peers that sync every few changes, delivered in six steps.  The
    default setting cuts its nodes at every change with a successor of the other peer; LM_CUT_MIN_ROWS=0 cuts every document's, a
    value above its size none."""
    rng = random.Random(5)
    a, b = wire.Replica(21), wire.Replica(22)
    order = []
    for i in range(380):
        r, o = (a, b) if rng.random() < 0.5 else (b, a)
        if rng.random() < 0.3:
            r.merge_from(o)
        name = "t%d" % r.peer
        for _ in range(3):   # (prepends: three op rows per change)
            r.text_insert(name, 0, "xy"); r.text_insert(name, len(r.seq[wire.root_cid(name, wire.KIND_TEXT)]), "z")
        r.commit()
        order.append(r.changes[r.peer][-1])
    assert sum(len(c.ops) for c in order) >= 2048
    cuts = [0, 70, 150, 151, 260, 330, len(order)]
    steps = []
    for lo, hi in zip(cuts, cuts[1:]):
        seg = order[lo:hi]
        steps.append((_p(*[c for c in seg if c.peer == 21]) + _p(*[c for c in seg if c.peer == 22]), None))
    G = "ImportGreaterUpdates"
    want = [(G, []), (G, [(21, 350), (22, 278)]), (G, [(21, 683), (22, 665)]), (G, [(21, 683), (22, 674)]), ("Import", []), ("Import", [])]
    return [LcaDoc("two peers, %d op rows" % sum(len(c.ops) for c in order), order, steps, want=want)]


def heap_docs():
    """the walk's heap holds 8 N + 64 spans (N nodes).  60 concurrent roots are resident; the step brings k changes of k new peers,
    each written on top of ALL 60 roots, and one more concurrent root.  Every one of the k heads is expanded before any root is
    popped (lamport 1 against 0) and pushes its 60 dependencies; equal spans are merged only when popped.  k = 60: 3,600 spans
    against 8 x 121 + 64 = 1,032 — the kernel gives up (-1) where the reference answers Import, [] (the new root is unmatched);
    k = 8: 480 against 8 x 69 + 64, answered.  So the overflow branch IS reachable by a legal history; it costs the answer, nothing
    else.  (After the step the version has k + 1 heads: an unchanged version of 61 heads is -1 by LCA_MAXF.)"""
    docs = []
    for k in (8, 60):
        roots = [wire.Replica(1000 + i) for i in range(60)]
        r0 = [_m(r) for r in roots]
        base = wire.Replica(1)
        for r in roots:
            base.merge_from(r)
        tops = []
        for j in range(k):
            r = wire.Replica(2000 + j)
            r.merge_from(base)
            tops.append(r)
        t0 = [_m(r) for r in tops]
        z = wire.Replica(5); z0 = _m(z)
        hs = sorted([(5, 0)] + [(2000 + j, 0) for j in range(k)])
        if k == 8:
            want = [("ImportGreaterUpdates", []), ("Import", [])] + [("Linear", hs)] * 4
            diff = []
        else:
            want = [("ImportGreaterUpdates", [])] + [UNKNOWN] * 5
            diff = [1, 2, 3, 4, 5]
        docs.append(LcaDoc("60 roots under %d heads" % k, _all(roots + tops + [z]), [(_p(*r0), None), (_p(*(t0 + [z0])), None)], want=want, oracle_differs=diff))
    return docs


def hand_groups():
    return {"after a failure": after_a_failure(), "fast exits": fast_exits(), "branches": branches(), "heads": many_heads(),
            "peers between steps": peers_between_steps(), "peer counts": peer_counts(), "heap": heap_docs(), "size": large()}


# ----------------------------------------------------------------------------------------------------------------------- corpus
SEEDS = {"flat": 60, "text": 40, "movable": 40}


def corpus(n_seeds=None):
    n = n_seeds or SEEDS
    docs = []
    for name in ("flat", "text", "movable"):
        for seed in range(n[name]):
            rng = random.Random(seed * 11 + 3)
            if name == "flat":
                reps = _fuzz.random_session(7000 + seed, n_peers=rng.randint(2, 5), n_steps=rng.randint(40, 100), kinds=("text", "list", "map"), styles=True, view=V)
            elif name == "text":
                reps = _fuzz.random_session(8000 + seed, n_peers=rng.randint(2, 4), n_steps=rng.randint(60, 120), kinds=("text",), max_ins=8, view=V)
            else:
                reps = _fuzz.movable_session(9000 + seed, n_peers=3, n_steps=80, nested=seed % 2 == 0, view=V)
            plan = _resident.plan_steps(_chunked(reps, rng), rng, N_STEPS)
            steps = [(ps, None, False) for ps, _ in plan]
            if seed % 5 == 0:   # one blob damaged; the whole step is delivered again with the next one
                at = [k for k in range(N_STEPS - 1) if steps[k][0]]
                if at:
                    k = rng.choice(at)
                    ps = steps[k][0]
                    j = rng.randrange(len(ps))
                    steps[k + 1] = (ps + steps[k + 1][0], None, False)
                    steps[k] = ([(damaged(b), cs) if i == j else (b, cs) for i, (b, cs) in enumerate(ps)], None, True)
            docs.append(LcaDoc("%s seed %d" % (name, seed), changes_of(reps), steps))
    return docs


# ----------------------------------------------------------------------------------------------------------------------- restatement
# dag.rs:487-765 (_find_common_ancestor_new with shrink_ancestor_frontiers and contains_in_ancestors) and the Import promotion of
# oplog.rs:610-615, over a list of plain node tuples (peer, first counter, atoms, lamport of the first atom, [dependency ids]).
# Written from the reference's text; it imports nothing of the oracle.
A, B, SHARED = 0, 1, 2


class _Dag:
    def __init__(self, nodes):
        self.by_peer = {}
        for n in nodes:
            self.by_peer.setdefault(n[0], []).append(n)
        for ns in self.by_peer.values():
            ns.sort(key=lambda n: n[1])

    def get(self, i):
        for n in self.by_peer.get(i[0], ()):
            if n[1] <= i[1] < n[1] + n[2]:
                return n
        return None

    def span(self, i):
        """OrdIdSpan::from_dag_node: (node, len) — the node's atoms up to `i`"""
        n = self.get(i)
        return None if n is None else (n, i[1] - n[1] + 1)


def _last(s):
    return (s[0][0], s[0][1] + s[1] - 1)


def _lam_last(s):
    return s[0][3] + s[1] - 1


def _contains(s, i):
    return s[0][0] == i[0] and s[0][1] <= i[1] < s[0][1] + s[1]


def _key(s):
    return (_lam_last(s), s[0][0], -s[1])          # Ord for OrdIdSpan, dag.rs:269-280: the shorter span is the greater


def _deps(dag, s):
    """deps_to_ord_id_spans (dag.rs:569-584); None when a dependency is not in the DAG"""
    out = []
    for d in s[0][4]:
        x = dag.span(tuple(d))
        if x is None:
            return None
        out.append(x)
    if s[0][1] > 0:
        prev = dag.span((s[0][0], s[0][1] - 1))
        if prev is not None and not any(_contains(d, _last(prev)) for d in out):
            out.append(prev)
    return out


def _in_ancestors(dag, frontier, target):
    visited, todo = set(), [dag.span(frontier)]
    while todo:
        s = todo.pop()
        if _contains(s, _last(target)):
            return True
        if _lam_last(s) < _lam_last(target):
            continue
        if (s[0][0], s[0][1]) in visited:
            continue
        visited.add((s[0][0], s[0][1]))
        todo += _deps(dag, s) or []
    return False


def _shrink(dag, ids):
    if len(ids) <= 1:
        return list(ids)
    spans = sorted((dag.span(i) for i in ids), key=_key)
    out = []
    for s in reversed(spans):
        if not any(_in_ancestors(dag, f, s) for f in reversed(out)):
            out.append(_last(s))
    return out


def find_common_ancestor(nodes, left, right):
    """-> (sorted ids, mode) as dag.rs:318-332 / 487-765 return them"""
    import heapq
    dag = _Dag(nodes)
    if not right:
        return [], "Checkout"
    if not left:
        if len(right) == 1:
            n = dag.get(right[0])
            while len(n[4]) == 1:
                n = dag.get(tuple(n[4][0]))
                if n is None:
                    return [], "ImportGreaterUpdates"
            if not n[4]:
                return [], "Linear"
        return [], "ImportGreaterUpdates"
    if len(left) == 1 and len(right) == 1 and left[0][0] == right[0][0]:
        l, r = left[0], right[0]
        ln, rn = dag.get(l), dag.get(r)
        if ln[1] == rn[1]:
            return ([l], "Linear") if l[1] < r[1] else ([r], "Checkout")
        if len(ln[4]) == 1 and _contains((rn, rn[2]), tuple(ln[4][0])):
            return [r], "Checkout"
        if len(rn[4]) == 1 and _contains((ln, ln[2]), tuple(rn[4][0])):
            return [l], "Linear"
    is_linear, right_greater, unmatched = len(left) <= 1 and len(right) == 1, True, False
    ans, heap, seq = [], [], [0]

    def push(s, t):
        k = _key(s)
        seq[0] += 1
        heapq.heappush(heap, ((-k[0], -k[1], -k[2], -t), seq[0], s, t))     # a max-heap over (span, type)
    for i in left:
        push(dag.span(i), A)
    for i in right:
        push(dag.span(i), B)
    while heap:
        _, _, s, t = heapq.heappop(heap)
        while heap:
            o, ot = heap[0][2], heap[0][3]
            if (o[0] is s[0] and o[1] == s[1]) or _last(o) == _last(s):
                if t != ot:
                    t = SHARED
                heapq.heappop(heap)
            else:
                break
        if t == SHARED:
            ans.append(_last(s))
            continue
        if not heap:
            unmatched, right_greater = True, False
            break
        if t == A:
            right_greater = False
        o, ot = heap[0][2], heap[0][3]
        if _contains(s, _last(o)) and t != ot:
            push((s[0], _last(o)[1] - s[0][1] + 1), t)
            continue
        if s[1] > 1:
            push((s[0], min(_lam_last(o) - s[0][3] + 1, s[1] - 1) if _lam_last(o) >= s[0][3] else 1), t)
            continue
        deps = _deps(dag, s)
        if deps is None:
            unmatched, right_greater = True, False
            continue
        if deps:
            for d in deps:
                push(d, t)
            is_linear = False
            continue
        unmatched, right_greater = True, False
    ans = _shrink(dag, ans)
    if unmatched:                                   # (no trimmed history in these documents: has_trimmed_history_deps is false)
        ans = []
    mode = ("Linear" if is_linear else "ImportGreaterUpdates") if right_greater else "Checkout"
    return sorted(ans), mode


# ---- node builders over the applied changes of a model (Model.changes: cut at the applied ends, in (lamport, peer, counter) order)
def never_cut(m):
    """what the oracle builds: a run of changes that depend on nothing but their peer's previous atom is one node"""
    nodes = []
    for p, chs in m.by_peer.items():
        cur = None
        for c in chs:
            if cur is not None and list(c.deps) == [(p, c.counter - 1)] and cur[1] + cur[2] == c.counter and cur[3] + cur[2] == c.lamport:
                cur[2] += c.ctr_end - c.counter
            else:
                cur = [p, c.counter, c.ctr_end - c.counter, c.lamport, [tuple(d) for d in c.deps]]
                nodes.append(cur)
    return [tuple(n) for n in nodes]


def cut_at_successors(m):
    """what k_dag_a builds under LM_CUT_MIN_ROWS=0: such a run is cut behind every change another peer's change depends on"""
    succ = {tuple(d) for c in m.changes for d in c.deps if d[0] != c.peer}
    nodes = []
    for p, chs in m.by_peer.items():
        cur = None
        for c in chs:
            if cur is not None and list(c.deps) == [(p, c.counter - 1)] and cur[1] + cur[2] == c.counter and cur[3] + cur[2] == c.lamport \
                    and (p, c.counter - 1) not in succ:
                cur[2] += c.ctr_end - c.counter
            else:
                cur = [p, c.counter, c.ctr_end - c.counter, c.lamport, [tuple(d) for d in c.deps]]
                nodes.append(cur)
    return [tuple(n) for n in nodes]


def every_change(m):
    """the finest partition: one node per change"""
    return [(c.peer, c.counter, c.ctr_end - c.counter, c.lamport, [tuple(d) for d in c.deps]) for c in m.changes]


def as_delivered(f):
    """the reference's own partition: `Delivered`, run beside the model in LcaDoc.facts()"""
    return f.nodes


PARTITIONS = {"never_cut": lambda f: never_cut(f.model), "cut_at_successors": lambda f: cut_at_successors(f.model), "as_delivered": as_delivered}


def restated(f, build):
    """(mode, L) of a step from the restatement over one partition of the model's applied changes (oplog.rs:610-615 promotion,
    diff_calc.rs:150-152 for an unchanged version)"""
    m = f.model
    hf, ht = f.heads_F, heads(m, f.T)
    if not f.grew:
        return "Linear", hf
    L, mode = find_common_ancestor(build(f), hf, ht)
    if mode == "Checkout":
        mode = "Import"                             # the version grew: to > from
    return mode, L
