"""Frontiers and version vectors (k_version, lm_frontiers / lm_versions): the expectation and the documents, shared by
tests/test_versions_ref.py (kernel-logic harness) and tests/test_gpu_zz_versions.py.

What a query must answer is stated over SETS OF IDS from the plain model (tests/_merge_ref.py: `Model.closure_of_id`, `Model.version`,
`Model.all_ids`) — closure(F) = the union of the ids' closures, heads(S) = the ids of S no other id of S has in its closure (`Ref.heads`,
written here) — and encoded by the postcard writers of this module (`enc_frontiers`, `enc_vv`; no oracle call, no wire.py encoder for
the expected bytes).  `hand_literals()` holds answers written out by hand, byte by byte, which the statement must reproduce first.

Corpus (`corpus()`): 30 fuzz sessions of the existing writers with their view from the model (text / list / map, 2-5 peers); the recorded
versions of a session are every snapshot frontier of the writers, every replica's own frontiers, two ids inside changes and the
frontiers of two replicas taken together.  Every version is asked all five ways (`version_queries`), plus a MINIMIZE over the version
and ids of its past, a TO_FRONTIERS of a vector that is NOT causally closed (one peer of the version's vector raised to a later
counter), a CMP against the next version, against itself with ids of its past added, and a CMP_DOC with an id nobody applied.
Counts over the corpus (from the model alone, asserted against FLOORS before any comparison; `counts`):
  queries 7,931 over 749 versions (186 of them with two or more ids);to_vv_extra_peer 569; to_frontiers_fewer_heads 1,127; to_frontiers_two_or_more 532;
  minimize_drops 795; cmp_less 1,012, cmp_equal 751, cmp_greater 827, cmp_concurrent 368; cmp_doc_less 262, cmp_doc_equal 43,
  cmp_doc_greater 706; not_closed 353.  Every floor is 100 but cmp_doc_equal's 20 (one latest version per session, and the versions
  that happen to be it).
Hand-built documents (`hand_docs()`, ONE batch of 17 documents, 1,235 queries with literal answers which the statement must give too):
1 / 2 / 63 / 64 / 65 / 255 concurrent roots with and without a merge change on top, asked with frontiers of 1 / 2 / 63 / 64 / 65 / 255
ids from both ends of the peer table; the same on peer ids 1, 2^32 - 1, 2^32, 2^63 - 1, 2^63, 2^64 - 1; a chain of four changes with a
reader of its middle (every counter of the node, against both atoms of the reader); pending changes; counters 2^24 - 2, 2^31 - 1 and
-1 as refused ids; one peer's 20,000 atoms asked at APPLIED counters of two and three encoded bytes; malformed bytes.
"""
import random

import _fuzz, _merge_ref
from _richtext_ref import changes_of
from loro_amd import wire

OK, DECODE_ERROR, UNSUPPORTED, NOT_FOUND = 0, 1, 4, 6
TO_VV, TO_FRONTIERS, MINIMIZE, CMP, CMP_DOC = range(5)
LESS, EQUAL, GREATER, CONCURRENT = -1, 0, 1, 2

FLOORS = {"to_vv_extra_peer": 100, "to_frontiers_fewer_heads": 100, "to_frontiers_two_or_more": 100, "minimize_drops": 100,
          "cmp_less": 100, "cmp_equal": 100, "cmp_greater": 100, "cmp_concurrent": 100,
          "cmp_doc_less": 100, "cmp_doc_equal": 20, "cmp_doc_greater": 100, "not_closed": 100}


# ---- postcard, written here: LEB128 u64, zigzag i32
def _uleb(n):
    assert n >= 0
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _zigzag(n):
    return _uleb((n << 1) ^ (n >> 31) if n >= 0 else ((-n) << 1) - 1)


def enc_frontiers(ids):
    """Frontiers::encode(): Vec<ID> sorted by (peer, counter)"""
    ids = sorted(set(ids))
    return _uleb(len(ids)) + b"".join(_uleb(p) + _zigzag(c) for p, c in ids)


def enc_vv(vv):
    """VersionVector::encode(): `vv` = {peer: counter} or [(peer, counter)] (kept as given, zeros included), ascending peers"""
    items = sorted(vv.items() if isinstance(vv, dict) else vv)
    return _uleb(len(items)) + b"".join(_uleb(p) + _zigzag(c) for p, c in items)


# ---- the statement
class Ref:
    def __init__(self, model):
        self.m = model
        self.end = {}
        for p, c in model.all_ids:
            self.end[p] = max(self.end.get(p, 0), c + 1)
        self._cl = {}

    def known(self, id):
        return id in self.m.all_ids

    def cl(self, id):
        if id not in self._cl:
            self._cl[id] = self.m.closure_of_id(id)
        return self._cl[id]

    def closure(self, ids):
        return frozenset().union(*[self.cl(i) for i in ids])

    def vv(self, ids):
        out = {}
        for p, c in self.closure(ids):
            out[p] = max(out.get(p, 0), c + 1)
        return out

    def heads(self, ids):
        ids = sorted(set(ids))
        return [i for i in ids if not any(i in self.cl(o) for o in ids if o != i)]

    def doc_heads(self):
        return self.heads([(p, e - 1) for p, e in self.end.items()])

    # (status, order, bytes) of a query
    def to_vv(self, ids):
        if not all(self.known(i) for i in ids):
            return (NOT_FOUND, 0, b"")
        return (OK, 0, enc_vv({p: c for p, c in self.vv(ids).items() if c > 0}))

    def to_frontiers(self, vv):
        ids = [(p, c - 1) for p, c in (vv.items() if isinstance(vv, dict) else vv) if c > 0]
        if not all(self.known(i) for i in ids):
            return (NOT_FOUND, 0, b"")
        return (OK, 0, enc_frontiers(self.heads(ids)))

    def minimize(self, ids):
        if not all(self.known(i) for i in ids):
            return (NOT_FOUND, 0, b"")
        return (OK, 0, enc_frontiers(self.heads(ids)))

    def cmp(self, a, b):
        if not all(self.known(i) for i in list(a) + list(b)):
            return (NOT_FOUND, 0, b"")
        A, B = self.closure(a), self.closure(b)
        return (OK, EQUAL if A == B else LESS if A < B else GREATER if A > B else CONCURRENT, b"")

    def cmp_doc(self, a):
        if set(a) == set(self.doc_heads()):
            return (OK, EQUAL, b"")
        if all(c >= 0 and c < self.end.get(p, 0) for p, c in a):
            return (OK, GREATER, b"")
        return (OK, LESS, b"")


class VDoc:
    """a document: its blobs, the model of what they apply, the versions it is asked at (lists of ids of the applied history)"""

    def __init__(self, label, changes, blobs, versions=(), delivered=None):
        self.label, self.changes, self.blobs = label, list(changes), list(blobs)
        self.model = _merge_ref.Model(self.changes, delivered=delivered)
        self.ref = Ref(self.model)
        self.versions = [sorted(set(v)) for v in versions]


def of_reps(label, reps, versions=(), blobs=None):
    return VDoc(label, changes_of(reps), blobs if blobs is not None else _fuzz.blobs_of(reps), versions)


# ---- hand literals: every byte written out by hand
def hand_literals():
    """peers 1 and 2 write three atoms each, concurrently (a fork); peer 3 merges both and writes two atoms (a merge change that
    dominates both).  -> (VDoc, [(query, (status, order, bytes))])"""
    a, b, c = wire.Replica(1), wire.Replica(2), wire.Replica(3)
    a.map_set("m", "a", 1); a.map_set("m", "b", 2); a.map_set("m", "c", 3); a.commit()
    b.map_set("m", "a", 4); b.map_set("m", "d", 5); b.map_set("m", "e", 6); b.commit()
    c.merge_from(a); c.merge_from(b)
    c.map_set("m", "f", 7); c.map_set("m", "g", 8); c.commit()
    d = of_reps("fork and merge", [a, b, c])
    H = bytes.fromhex
    lit = [
        # the empty version, both ways
        ((0, TO_VV, H("00")), (OK, 0, H("00"))),
        ((0, TO_FRONTIERS, H("00")), (OK, 0, H("00"))),
        ((0, MINIMIZE, H("00")), (OK, 0, H("00"))),
        # the fork: [1@2, 2@2] <-> {1: 3, 2: 3}
        ((0, TO_VV, H("02 01 04 02 04")), (OK, 0, H("02 01 06 02 06"))),
        ((0, TO_FRONTIERS, H("02 01 06 02 06")), (OK, 0, H("02 01 04 02 04"))),
        ((0, MINIMIZE, H("02 01 04 02 04")), (OK, 0, H("02 01 04 02 04"))),
        ((0, CMP, H("01 01 04"), H("01 02 04")), (OK, CONCURRENT, b"")),
        # the merge change dominates both: 3@1 <-> {1: 3, 2: 3, 3: 2}; 3@0 holds both heads already
        ((0, TO_VV, H("01 03 02")), (OK, 0, H("03 01 06 02 06 03 04"))),
        ((0, TO_VV, H("01 03 00")), (OK, 0, H("03 01 06 02 06 03 02"))),
        ((0, TO_FRONTIERS, H("03 01 06 02 06 03 04")), (OK, 0, H("01 03 02"))),
        ((0, MINIMIZE, H("03 01 04 02 04 03 00")), (OK, 0, H("01 03 00"))),
        ((0, CMP, H("01 03 00"), H("02 01 04 02 04")), (OK, GREATER, b"")),
        ((0, CMP, H("02 01 04 02 04"), H("01 03 02")), (OK, LESS, b"")),
        ((0, CMP, H("03 01 04 02 04 03 02"), H("01 03 02")), (OK, EQUAL, b"")),
        # an id in the middle of a run: 1@1 <-> {1: 2}; 3@0 in the middle of the merge change
        ((0, TO_VV, H("01 01 02")), (OK, 0, H("01 01 04"))),
        ((0, TO_FRONTIERS, H("01 01 04")), (OK, 0, H("01 01 02"))),
        ((0, CMP, H("01 01 02"), H("01 01 04")), (OK, LESS, b"")),
        ((0, MINIMIZE, H("02 01 02 01 04")), (OK, 0, H("01 01 04"))),             # two ids of one peer: the greater
        ((0, TO_FRONTIERS, H("02 01 04 02 06")), (OK, 0, H("02 01 02 02 04"))),   # {1: 2, 2: 3}
        # a vector that is not closed: {3: 1} alone names 3@0, whose past is not in the vector — the shrink of the last ids keeps it
        ((0, TO_FRONTIERS, H("01 03 02")), (OK, 0, H("01 03 00"))),
        ((0, TO_FRONTIERS, H("02 01 02 03 02")), (OK, 0, H("01 03 00"))),         # {1: 1, 3: 1}: 1@0 lies in the past of 3@0
        # against the document
        ((0, CMP_DOC, H("01 03 02")), (OK, EQUAL, b"")),
        ((0, CMP_DOC, H("02 01 04 02 04")), (OK, GREATER, b"")),
        ((0, CMP_DOC, H("01 03 04")), (OK, LESS, b"")),                            # 3@2: one past the end
        ((0, CMP_DOC, H("01 09 00")), (OK, LESS, b"")),                            # an unknown peer: no error
        ((0, CMP_DOC, H("00")), (OK, GREATER, b"")),
        # refused ids
        ((0, TO_VV, H("01 03 04")), (NOT_FOUND, 0, b"")),
        ((0, TO_VV, H("01 09 00")), (NOT_FOUND, 0, b"")),
        ((0, TO_VV, H("01 01 01")), (NOT_FOUND, 0, b"")),                          # 1@-1
        ((0, MINIMIZE, H("02 01 04 09 00")), (NOT_FOUND, 0, b"")),
        ((0, CMP, H("01 01 04"), H("01 09 00")), (NOT_FOUND, 0, b"")),
        ((0, TO_FRONTIERS, H("01 03 06")), (NOT_FOUND, 0, b"")),                   # {3: 3}
        ((0, TO_FRONTIERS, H("01 09 0a")), (NOT_FOUND, 0, b"")),                   # {9: 5}: an unknown peer above 0
        ((0, TO_FRONTIERS, H("02 01 04 09 00")), (OK, 0, H("01 01 02"))),          # {1: 2, 9: 0}: an entry of 0 is skipped
    ]
    return d, lit


def decode(query):
    """the ids / entries of a query's bytes (this module's reader: the inverse of the writers above; raises on anything else)"""
    def rd(b):
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
        assert i == len(b)
        return out
    return [rd(x) for x in query[2:]]


def answer(ref, query):
    """the statement's answer to a well-formed query"""
    ids = decode(query)
    op = query[1]
    if op == TO_VV:
        return ref.to_vv(ids[0])
    if op == TO_FRONTIERS:
        return ref.to_frontiers(ids[0])
    if op == MINIMIZE:
        return ref.minimize(ids[0])
    if op == CMP:
        return ref.cmp(ids[0], ids[1])
    return ref.cmp_doc(ids[0])


# ---- corpus
SEEDS = list(range(4100, 4130))


def _versions_of(reps, snaps, rng):
    out, seen = [], set()

    def add(fr):
        key = tuple(sorted(set(fr)))
        if key and key not in seen:
            seen.add(key); out.append(list(key))
    for fr, _ in snaps:
        add(fr)
    for r in reps:
        add(r.frontiers)
    own = [(r, r.changes.get(r.peer, [])) for r in reps if r.changes.get(r.peer)]
    for _ in range(2):                                   # an id inside a change
        r, chs = rng.choice(own)
        ch = rng.choice(chs)
        add([(r.peer, rng.randrange(ch.counter, ch.ctr_end))])
    for _ in range(3):                                   # the frontiers of two replicas together: not minimal, as a rule
        a, b = rng.sample(reps, 2) if len(reps) > 1 else (reps[0], reps[0])
        add(list(a.frontiers) + list(b.frontiers))
    if snaps:
        for _ in range(3):                               # … and of two recorded versions
            add(list(rng.choice(snaps)[0]) + list(rng.choice(snaps)[0]))
    return out


def corpus(seeds=SEEDS):
    docs = []
    for seed in seeds:
        rng = random.Random(seed)
        snaps = []
        reps = _fuzz.random_session(seed, n_peers=2 + seed % 4, n_steps=70 + 10 * (seed % 3), kinds=[("text", "map"), ("text", "list", "map"), ("map",)][seed % 3],
                                    sync_prob=0.2, view=_merge_ref.view, snapshots=snaps)
        d = of_reps("fuzz %d" % seed, reps, _versions_of(reps, snaps, rng))
        d.versions.append(d.ref.doc_heads())             # the latest version
        docs.append(d)
    return docs


def version_queries(k, d, seed=0):
    """every version of document `d` (index k in its batch) all five ways -> [(query, want, tag)]"""
    rng = random.Random(seed * 7919 + k)
    ref = d.ref
    out = []
    peers = sorted(ref.end)
    for vi, F in enumerate(d.versions):
        G = d.versions[(vi + 1) % len(d.versions)]
        vv = ref.vv(F)
        past = sorted(ref.closure(F) - set(F))
        extra = rng.sample(past, min(len(past), rng.randint(1, 4)))
        out.append(((k, TO_VV, enc_frontiers(F)), ref.to_vv(F), "to_vv"))
        out.append(((k, TO_FRONTIERS, enc_vv(vv)), ref.to_frontiers(vv), "to_frontiers"))
        out.append(((k, MINIMIZE, enc_frontiers(F)), ref.minimize(F), "minimize"))
        out.append(((k, MINIMIZE, enc_frontiers(F + extra)), ref.minimize(F + extra), "minimize"))
        out.append(((k, CMP, enc_frontiers(F), enc_frontiers(G)), ref.cmp(F, G), "cmp"))
        out.append(((k, CMP, enc_frontiers(F + extra), enc_frontiers(F)), ref.cmp(F + extra, F), "cmp"))
        if extra:
            out.append(((k, CMP, enc_frontiers(extra[:1]), enc_frontiers(F)), ref.cmp(extra[:1], F), "cmp"))
            out.append(((k, CMP, enc_frontiers(F), enc_frontiers(extra[:1])), ref.cmp(F, extra[:1]), "cmp"))
        out.append(((k, CMP_DOC, enc_frontiers(F)), ref.cmp_doc(F), "cmp_doc"))
        if vi % 3 == 0:                                   # an id nobody applied: one past a peer's end / an unknown peer
            p = rng.choice(peers)
            bad = F + [(p, ref.end[p])] if vi % 2 == 0 else F + [(max(peers) + 1 + vi, 0)]
            out.append(((k, CMP_DOC, enc_frontiers(bad)), ref.cmp_doc(bad), "cmp_doc"))
            out.append(((k, TO_VV, enc_frontiers(bad)), ref.to_vv(bad), "refused"))
        # a vector that is not causally closed: one peer raised beyond what the version holds
        room = [p for p in peers if vv.get(p, 0) < ref.end[p]]
        if room:
            p = rng.choice(room)
            up = dict(vv); up[p] = rng.randint(vv.get(p, 0) + 1, ref.end[p])
            closed = ref.vv([(q, c - 1) for q, c in up.items()]) == up
            out.append(((k, TO_FRONTIERS, enc_vv(up)), ref.to_frontiers(up), "closed" if closed else "not_closed"))
    return out


def counts(docs, queries):
    """FLOORS' quantities of `queries` = [(query, want, tag)], from the statement alone"""
    tot = dict.fromkeys(FLOORS, 0)
    for q, w, tag in queries:
        if w[0] != OK:
            continue
        ids = decode(q)
        if q[1] == TO_VV:
            tot["to_vv_extra_peer"] += bool({p for p, c in decode((0, 0, w[2]))[0]} - {p for p, _ in ids[0]})
        elif q[1] == TO_FRONTIERS:
            n_heads, n_in = len(decode((0, 0, w[2]))[0]), sum(1 for _, c in ids[0] if c > 0)
            tot["to_frontiers_fewer_heads"] += n_heads < n_in
            tot["to_frontiers_two_or_more"] += n_heads >= 2
            tot["not_closed"] += tag == "not_closed"
        elif q[1] == MINIMIZE:
            tot["minimize_drops"] += len(decode((0, 0, w[2]))[0]) < len(set(ids[0]))
        elif q[1] == CMP:
            tot[{LESS: "cmp_less", EQUAL: "cmp_equal", GREATER: "cmp_greater", CONCURRENT: "cmp_concurrent"}[w[1]]] += 1
        else:
            tot[{LESS: "cmp_doc_less", EQUAL: "cmp_doc_equal", GREATER: "cmp_doc_greater"}[w[1]]] += 1
    return tot


def check_floors(tot, floors=FLOORS, scale=1):
    for k, least in floors.items():
        assert tot[k] >= max(20 if k != "not_closed" else 10, least // scale), (k, tot)


# ---- running
def check(ctx, queries, what=""):
    """one lm_versions call for `queries` = [(query, want, …)]; -> the number compared"""
    got = ctx.versions([q[0] for q in queries])
    assert len(got) == len(queries)
    for g, q in zip(got, queries):
        assert g == q[1], (what, q[0][:2], [x.hex() for x in q[0][2:]], "got", (g[0], g[1], g[2].hex()), "want", (q[1][0], q[1][1], q[1][2].hex()))
    return len(got)


def check_heads(ctx, k, d, rendered=None, what=""):
    """lm_frontiers both ways for document k: everything applied, and the rendered version (`rendered` = the frontiers given, None = latest)"""
    want = enc_frontiers(d.ref.doc_heads())
    got = ctx.frontiers(k, 0)
    assert got == want, (what, d.label, "which 0", got and got.hex(), want.hex())
    want1 = want if rendered is None else enc_frontiers(d.ref.heads(rendered))
    got = ctx.frontiers(k, 1)
    assert got == want1, (what, d.label, "which 1", got and got.hex(), want1.hex())


def run_latest(ctx, docs, queries, what=""):
    """the documents as one batch at their latest version: results, heads, the queries in one call, results again"""
    res = ctx.merge_batch([d.blobs for d in docs])
    assert res == [d.model.result() for d in docs], what
    for k, d in enumerate(docs):
        check_heads(ctx, k, d, None, what)
    n = check(ctx, queries, what)
    assert ctx.fetch() == res, what
    return n


# ---- hand-built documents on the kernel's boundaries
EDGE_PEERS = [1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]


def roots_doc(peers, merge):
    """one concurrent root change of two atoms per peer; `merge`: the first peer then takes all of them in and writes three atoms on top"""
    reps = [wire.Replica(p) for p in peers]
    for i, r in enumerate(reps):
        r.map_set("m", "k%d" % (i % 7), i); r.map_set("m", "j%d" % (i % 5), -i); r.commit()
    if merge:
        for r in reps[1:]:
            reps[0].merge_from(r)
        reps[0].map_set("m", "top", 1); reps[0].map_set("m", "top", 2); reps[0].map_set("m", "top", 3); reps[0].commit()
    return of_reps("%d roots%s" % (len(peers), ", merged" if merge else ""), reps)


def roots_queries(k, d, peers, merge):
    """frontiers of 1 / 2 / 63 / 64 / 65 / 255 of the roots (as many as the document has), with literal answers: the roots are pairwise
    concurrent, so k of them are their own heads and their vector is {p: 2} over exactly those peers; the merge change dominates all"""
    out = []
    n = len(peers)
    p0 = peers[0]
    for m in [x for x in (1, 2, 63, 64, 65, 255) if x <= n]:
        for sub in (peers[:m], peers[n - m:]):
            F = [(p, 1) for p in sub]
            vv = enc_vv({p: 2 for p in sub})
            fr = enc_frontiers(F)
            out.append(((k, TO_VV, fr), (OK, 0, vv)))
            out.append(((k, TO_FRONTIERS, vv), (OK, 0, fr)))
            out.append(((k, MINIMIZE, fr), (OK, 0, fr)))
            out.append(((k, MINIMIZE, enc_frontiers(F + [(p, 0) for p in sub])), (OK, 0, fr)))           # first and last counter of every root
            out.append(((k, TO_VV, enc_frontiers([(p, 0) for p in sub])), (OK, 0, enc_vv({p: 1 for p in sub}))))
            if merge:
                top = [(p0, 2), (p0, 3), (p0, 4)]
                for t in top:
                    out.append(((k, CMP, fr, enc_frontiers([t])), (OK, LESS, b"")))
                    out.append(((k, MINIMIZE, enc_frontiers(F + [t])), (OK, 0, enc_frontiers([t]))))
                out.append(((k, CMP_DOC, fr), (OK, GREATER, b"")))
            else:
                out.append(((k, CMP_DOC, fr), (OK, EQUAL if m == n else GREATER, b"")))
                if m < n:
                    other = [(p, 1) for p in peers if p not in sub][:m]
                    out.append(((k, CMP, fr, enc_frontiers(other)), (OK, CONCURRENT if sub[0] not in [p for p, _ in other] else EQUAL, b"")))
                    out.append(((k, CMP, fr, enc_frontiers(F + other)), (OK, LESS, b"")))
    if merge:
        all_vv = {p: 2 for p in peers}
        for c in (2, 3, 4):
            all_vv[p0] = c + 1
            out.append(((k, TO_VV, enc_frontiers([(p0, c)])), (OK, 0, enc_vv(all_vv))))
            out.append(((k, TO_FRONTIERS, enc_vv(all_vv)), (OK, 0, enc_frontiers([(p0, c)]))))
        out.append(((k, CMP_DOC, enc_frontiers([(p0, 4)])), (OK, EQUAL, b"")))
        out.append(((k, CMP_DOC, enc_frontiers([(p0, 3)])), (OK, GREATER, b"")))
    # ids nobody applied
    out.append(((k, TO_VV, enc_frontiers([(peers[-1], 5 if merge and n == 1 else 2)])), (NOT_FOUND, 0, b"")))   # one past the applied end
    out.append(((k, TO_VV, enc_frontiers([(peers[-1], (1 << 24) - 2)])), (NOT_FOUND, 0, b"")))
    out.append(((k, TO_VV, enc_frontiers([(peers[-1], -1)])), (NOT_FOUND, 0, b"")))
    out.append(((k, TO_VV, enc_frontiers([(peers[0], (1 << 31) - 1)])), (NOT_FOUND, 0, b"")))
    return out


def chain_doc():
    """peer 20 writes four changes in a row (3, 2, 2 and 2 atoms: one DAG node unless it is cut); peer 10 has seen the first two (20@0..4)
    and writes two atoms; peer 20 never sees peer 10.  Asked at the first / a middle / the last counter of the node and of every change
    inside it; LM_CUT_MIN_ROWS=0 cuts the node behind 20@4 -> (VDoc, [(query, literal)])"""
    b = wire.Replica(10)
    a2 = wire.Replica(20)
    a2.map_set("m", "x", 0); a2.map_set("m", "x", 1); a2.map_set("m", "x", 2); a2.commit()
    a2.map_set("m", "y", 0); a2.map_set("m", "y", 1); a2.commit()
    b.merge_from(a2)
    b.map_set("m", "z", 1); b.map_set("m", "z", 2); b.commit()
    a2.map_set("m", "y", 2); a2.map_set("m", "y", 3); a2.commit()
    a2.map_set("m", "w", 0); a2.map_set("m", "w", 1); a2.commit()
    d = of_reps("a chain and a reader of its middle", [a2, b])
    k = 0
    out = []
    for c in range(9):                                   # 20@0..8: the change [0,3), [3,5), [5,7), [7,9)
        out.append(((k, TO_VV, enc_frontiers([(20, c)])), (OK, 0, enc_vv({20: c + 1}))))
        out.append(((k, TO_FRONTIERS, enc_vv({20: c + 1})), (OK, 0, enc_frontiers([(20, c)]))))
        for z in (0, 1):                                 # against 10@z, which holds 20@0..4
            order = LESS if c <= 4 else CONCURRENT
            out.append(((k, CMP, enc_frontiers([(20, c)]), enc_frontiers([(10, z)])), (OK, order, b"")))
            out.append(((k, MINIMIZE, enc_frontiers([(20, c), (10, z)])), (OK, 0, enc_frontiers([(10, z)] if c <= 4 else [(10, z), (20, c)]))))
            out.append(((k, TO_VV, enc_frontiers([(20, c), (10, z)])), (OK, 0, enc_vv({10: z + 1, 20: max(c + 1, 5)}))))
            out.append(((k, TO_FRONTIERS, enc_vv({10: z + 1, 20: c + 1})), (OK, 0, enc_frontiers([(10, z)] if c <= 4 else [(10, z), (20, c)]))))
    out.append(((k, CMP_DOC, enc_frontiers([(10, 1), (20, 8)])), (OK, EQUAL, b"")))
    out.append(((k, CMP_DOC, enc_frontiers([(10, 1), (20, 7)])), (OK, GREATER, b"")))
    return d, out


def pending_doc():
    """peer 5 delivers its first and its third change: the third is pending.  Peer 6 delivers a change that depends on the missing one:
    pending too -> (VDoc, [(query, literal)])"""
    a, b = wire.Replica(5), wire.Replica(6)
    a.map_set("m", "a", 1); a.map_set("m", "a", 2); a.commit()
    a.map_set("m", "b", 1); a.commit()
    b.merge_from(a)
    b.map_set("m", "c", 1); b.commit()
    a.map_set("m", "d", 1); a.map_set("m", "d", 2); a.commit()
    chs = a.changes[5]
    first, third = wire.Replica(5), wire.Replica(5)
    first.changes = {5: [chs[0]]}; third.changes = {5: [chs[2]]}
    own_b = wire.Replica(6); own_b.changes = {6: b.changes[6]}
    blobs = [first.export(), wire.encode_updates([[chs[2]]]), own_b.export()]
    d = VDoc("pending changes", changes_of([a, b]), blobs, delivered=[chs[0], chs[2]] + b.changes[6])
    assert d.model.pending == 3 and d.ref.end == {5: 2}
    k = 0
    out = [((k, TO_VV, enc_frontiers([(5, 1)])), (OK, 0, enc_vv({5: 2}))),
           ((k, TO_VV, enc_frontiers([(5, 2)])), (NOT_FOUND, 0, b"")),          # one past the applied end (delivered by nobody)
           ((k, TO_VV, enc_frontiers([(5, 3)])), (NOT_FOUND, 0, b"")),          # inside a pending change
           ((k, TO_VV, enc_frontiers([(6, 0)])), (NOT_FOUND, 0, b"")),          # a pending change of a peer with nothing applied
           ((k, MINIMIZE, enc_frontiers([(5, 1), (5, 4)])), (NOT_FOUND, 0, b"")),
           ((k, CMP, enc_frontiers([(5, 0)]), enc_frontiers([(6, 0)])), (NOT_FOUND, 0, b"")),
           ((k, TO_FRONTIERS, enc_vv({5: 2, 6: 0})), (OK, 0, enc_frontiers([(5, 1)]))),
           ((k, TO_FRONTIERS, enc_vv({5: 2, 6: 1})), (NOT_FOUND, 0, b"")),
           ((k, TO_FRONTIERS, enc_vv({5: 5})), (NOT_FOUND, 0, b"")),
           ((k, CMP_DOC, enc_frontiers([(5, 1)])), (OK, EQUAL, b"")),
           ((k, CMP_DOC, enc_frontiers([(5, 4)])), (OK, LESS, b"")),
           ((k, CMP_DOC, enc_frontiers([(6, 0)])), (OK, LESS, b""))]
    return d, out


def long_doc():
    """one peer, 20,000 atoms in three changes (100, 8,900 and 11,000 atoms): APPLIED ids whose counters take two and three bytes in
    both encodings (zigzag: from 64 and from 8,192 on; a vector's counter + 1 likewise), at change edges and inside
    -> (VDoc, [(query, literal)])"""
    a = wire.Replica(77)
    for lo, hi in ((0, 100), (100, 9000), (9000, 20000)):
        for i in range(lo, hi):
            a.map_set("m", "k%d" % (i % 8), i)
        a.commit()
    d = of_reps("20,000 atoms of one peer", [a])
    assert d.ref.end == {77: 20000}
    k = 0
    out = []
    for c in (63, 64, 99, 100, 8190, 8191, 8192, 8999, 9000, 16383, 16384, 19998, 19999):
        fr, vv = enc_frontiers([(77, c)]), enc_vv({77: c + 1})
        assert len(fr) == (3 if c < 64 else 4 if c < 8192 else 5)
        out.append(((k, TO_VV, fr), (OK, 0, vv)))
        out.append(((k, TO_FRONTIERS, vv), (OK, 0, fr)))
        out.append(((k, MINIMIZE, enc_frontiers([(77, c), (77, 5), (77, c - 1)])), (OK, 0, fr)))
        out.append(((k, CMP, fr, enc_frontiers([(77, 16384)])), (OK, LESS if c < 16384 else EQUAL if c == 16384 else GREATER, b"")))
        out.append(((k, CMP_DOC, fr), (OK, EQUAL if c == 19999 else GREATER, b"")))
    out.append(((k, TO_VV, enc_frontiers([(77, 20000)])), (NOT_FOUND, 0, b"")))
    out.append(((k, TO_FRONTIERS, enc_vv({77: 20001})), (NOT_FOUND, 0, b"")))
    return d, out


def malformed_queries(k):
    """bytes that are neither: truncated, bytes left over, a counter beyond 32 bits, zero length; and the well-formed neighbours"""
    H = bytes.fromhex
    bad = [H("01"), H("01 01"), H("02 01 02"), H("01 01 02 00"), H("00 00"), H("01 01 ff ff ff ff 7f"), H("ff"), b"", H("01 80")]
    out = []
    for b in bad:
        for op in (TO_VV, TO_FRONTIERS, MINIMIZE, CMP_DOC):
            out.append(((k, op, b), (DECODE_ERROR, 0, b"")))
        out.append(((k, CMP, b, H("00")), (DECODE_ERROR, 0, b"")))
        out.append(((k, CMP, H("00"), b), (DECODE_ERROR, 0, b"")))
    out.append(((k, CMP, H("00"), H("00")), (OK, EQUAL, b"")))
    out.append(((k, TO_VV, H("00")), (OK, 0, H("00"))))
    return out


def hand_docs():
    """-> (docs, [(query, literal want)]) for ONE batch: peer counts on the lane strides with and without a merge on top, the edge
    peer ids, the chain, the pending changes; the literals are checked against the statement by the caller"""
    docs, qs = [], []
    for n in (1, 2, 63, 64, 65, 255):
        peers = [1000 + 3 * i for i in range(n)]
        for merge in (False, True):
            d = roots_doc(peers, merge)
            qs += roots_queries(len(docs), d, peers, merge)
            docs.append(d)
    for merge in (False, True):
        d = roots_doc(EDGE_PEERS, merge)
        qs += roots_queries(len(docs), d, EDGE_PEERS, merge)
        docs.append(d)
    for build in (chain_doc, pending_doc, long_doc):
        d, q = build()
        k = len(docs)
        qs += [((k,) + x[0][1:], x[1]) for x in q]
        docs.append(d)
    qs += malformed_queries(0)
    return docs, qs


def check_literals_against_the_statement(docs, qs):
    """every literal of a well-formed query is what the statement says"""
    n = 0
    for q, w in qs:
        if w[0] == DECODE_ERROR:
            continue
        got = answer(docs[q[0]].ref, q)
        assert got == w, (docs[q[0]].label, q[:2], [x.hex() for x in q[2:]], got, w)
        n += 1
    return n


def run_mixed(ctx, docs, what=""):
    """ONE batch in which every document has an entry WITHOUT a checkout and an entry WITH one, on a context whose previous batch —
    other documents, all checked out — left its own values in every table: an entry at its latest version has no applied ends of
    its own beside the rendered ones (k_dag_b writes them for checked-out entries only), and must not read anybody's stale ones"""
    other = list(reversed(docs))
    ctx.merge_batch([d.blobs for d in other], [wire.encode_frontiers(d.versions[0]) for d in other])
    blobs, fronts, given, owner = [], [], [], []
    for k, d in enumerate(docs):
        for F in (None, d.versions[k % len(d.versions)]):
            blobs.append(d.blobs); fronts.append(None if F is None else wire.encode_frontiers(F)); given.append(F); owner.append(k)
    res = ctx.merge_batch(blobs, fronts)
    qs = []
    for i, (k, F) in enumerate(zip(owner, given)):
        assert res[i] == docs[k].model.result(F), (what, docs[k].label, F)
        qs += [((i,) + q[0][1:], q[1]) for q in version_queries(k, docs[k])[:60]]
    for i, (k, F) in enumerate(zip(owner, given)):
        check_heads(ctx, i, docs[k], F, what)
    n = check(ctx, qs, what)
    assert ctx.fetch() == res, what
    return n


def shuffled(queries, seed=5):
    qs = list(queries)
    random.Random(seed).shuffle(qs)
    return qs
