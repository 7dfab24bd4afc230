"""Richtext values (lm_richtext): cases shared by the kernel-logic (CPU) and the GPU tests.  The checker is the
oracle's Doc::to_richtext (oracle/lo_doc.hpp), itself pinned on the reference's known answers below."""
import json
import random

import _fuzz, _oracle, _resident
from loro_amd import wire


def known_answers():
    """[(name, blobs, expected richtext value of root Text "text" as Python data)] — reference tests restated through the blob
    writer (wire.Replica places the anchors where TextHandler::mark places them for a plain range: StyleStart in front of the
    first scalar, StyleEnd behind the last, handler.rs mark_with_transaction):
      crates/loro/tests/loro_rust_test.rs:448-474 richtext_test (mark, then unmark 3..5 = a mark with value null)
      crates/loro/tests/loro_rust_test.rs:476-498 sync (the mark arrives as an update of another peer)
      crates/loro/src/lib.rs:2750-2772 get_richtext_value doc example"""
    out = []
    d = wire.Replica(1)
    d.text_insert("text", 0, "Hello world!"); d.text_mark("text", 0, 5, "bold", True); d.commit()
    out.append(("richtext_test: mark", [d.export()], [{"insert": "Hello", "attributes": {"bold": True}}, {"insert": " world!"}]))
    # unmark(3..5): scalars 3..5 sit behind the first Start anchor → entities 4..6
    d.text_mark("text", 4, 6, "bold", None); d.commit()
    out.append(("richtext_test: unmark", [d.export()], [{"insert": "Hel", "attributes": {"bold": True}}, {"insert": "lo world!"}]))
    a, b = wire.Replica(1), wire.Replica(2)
    a.text_insert("text", 0, "Hello world!"); a.commit()
    b.merge_from(a)
    b.set_visible("text", wire.KIND_TEXT, _oracle.visible_ids([a.export()], "text", wire.KIND_TEXT))
    b.text_mark("text", 0, 5, "bold", True); b.commit()
    own = wire.Replica(2); own.changes = {2: b.changes[2]}
    out.append(("sync", [a.export(), own.export()], [{"insert": "Hello", "attributes": {"bold": True}}, {"insert": " world!"}]))
    e = wire.Replica(3)
    e.text_insert("text", 0, "Hello world!"); e.text_mark("text", 0, 5, "bold", True); e.commit()
    out.append(("doc example", [e.export()], [{"insert": "Hello", "attributes": {"bold": True}}, {"insert": " world!"}]))
    return out


def reference_held():
    """[(name, blobs, expected richtext value of root Text "text")] — answers the REFERENCE's own tests hold for blobs it ships
    (unlike known_answers(), nothing here goes through this repo's writer): crates/loro/tests/loro_js_interop.rs:86-94 asserts
    `doc.get_text("text").get_richtext_value()` of runtime-snapshot.ts.blob == [{"insert":"b","attributes":{"bold":true}}] and
    (`to_delta()` equality, :86-89) the same spans for runtime-updates.ts.blob.  The blobs come from
    tests/golden/reference_fixtures.json (make_reference_fixtures.py).  Both documents also hold Tree / Counter containers, so
    their status is LM_UNSUPPORTED (4) with everything in scope rendered."""
    import os
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures.json")))["blobs"]
    want = [{"insert": "b", "attributes": {"bold": True}}]
    return [(n, [bytes.fromhex(fx[n])], want) for n in ("runtime-snapshot.ts.blob", "runtime-updates.ts.blob")]


def _hand():
    """[(name, blobs, the replicas that hold the changes)] — shapes the rule has to get right: two peers mark the same range concurrently (greater (lamport, peer)
    decides), overlapping marks of different keys, a mark whose End anchor was deleted / whose Start anchor was deleted,
    text typed inside and at both edges of a range, an unmark over part of a range, equal values from different ops (one span),
    several Text containers (a child Text in a Map, a Text without any visible scalar, a Text that holds only anchors)."""
    out = []   # (name, blobs, the replicas that hold the changes)
    a, b = wire.Replica(10), wire.Replica(20)
    a.text_insert("text", 0, "0123456789"); a.commit()
    b.merge_from(a); b.set_visible("text", wire.KIND_TEXT, _oracle.visible_ids([a.export()], "text", wire.KIND_TEXT))
    a.text_mark("text", 2, 6, "color", "red"); a.commit()
    b.text_mark("text", 4, 8, "color", "blue"); b.text_mark("text", 0, 3, "bold", True); b.commit()
    out.append(("concurrent marks of one key", _fuzz.blobs_of([a, b]), [a, b]))
    c = wire.Replica(5)
    c.text_insert("text", 0, "abcdefgh"); c.text_mark("text", 1, 5, "bold", True); c.commit()
    c.text_delete("text", 6, 1); c.commit()      # the End anchor (entity 6: a b c d e | End) … entity positions: 0 a,1 S,2 b..5 e,6 E
    out.append(("end anchor deleted", [c.export()], [c]))
    c2 = wire.Replica(6)
    c2.text_insert("text", 0, "abcdefgh"); c2.text_mark("text", 1, 5, "bold", True); c2.commit()
    c2.text_delete("text", 1, 1); c2.commit()    # the Start anchor
    out.append(("start anchor deleted", [c2.export()], [c2]))
    t = wire.Replica(7)
    t.text_insert("text", 0, "abcd"); t.text_mark("text", 1, 3, "bold", True); t.commit()   # a S b c E d
    t.text_insert("text", 3, "X"); t.text_insert("text", 1, "L"); t.text_insert("text", 7, "R"); t.commit()
    out.append(("typing inside and at the edges", [t.export()], [t]))
    u = wire.Replica(8)
    u.text_insert("text", 0, "abcdef"); u.text_mark("text", 0, 6, "link", "u1"); u.text_mark("text", 3, 5, "link", "u1"); u.text_mark("text", 1, 2, "em", 1); u.commit()
    out.append(("equal values from different ops", [u.export()], [u]))
    n = wire.Replica(9)
    n.map_set("m", "k", 1); n.text_insert("empty", 0, "zz"); n.text_delete("empty", 0, 2); n.text_insert("t2", 0, "plain \"text\"\n"); n.commit()
    n.text_insert("only_anchors", 0, "q"); n.text_mark("only_anchors", 0, 1, "b", True); n.text_delete("only_anchors", 1, 1); n.commit()
    out.append(("several text containers", [n.export()], [n]))
    return out


def hand_cases():
    return [(name, blobs) for name, blobs, _ in _hand()]


def hand_sessions():
    """[(name, replicas)] of hand_cases(): the writers' Change / Op objects, for the plain reference (tests/_richtext_ref.py)"""
    return [(name, reps) for name, _, reps in _hand()]


def fuzz_sessions(n, base=5000, n_steps=90, **kw):
    """the replicas of fuzz_docs()"""
    return [_fuzz.random_session(base + s, n_peers=2 + s % 3, n_steps=n_steps, kinds=("text",) if s % 3 else ("text", "list", "map"),
                                 styles="rich", sync_prob=0.1, **kw) for s in range(n)]


def fuzz_docs(n, base=5000, n_steps=90, **kw):
    return [_fuzz.blobs_of(reps) for reps in fuzz_sessions(n, base, n_steps, **kw)]


def nested_sessions(n, base=5200):
    """the replicas of nested_docs()"""
    return [_fuzz.nested_session(base + s, n_peers=3, n_steps=120) for s in range(n)]


def nested_docs(n, base=5200):
    return [_fuzz.blobs_of(reps) for reps in nested_sessions(n, base)]


def checkout_cases(n=6, base=5400):
    """(docs, frontiers): every few recorded versions of rich sessions, incl. versions that cut a StyleStart from its StyleEnd"""
    docs, fronts = [], []
    for s in range(n):
        snaps = []
        reps = _fuzz.random_session(base + s, n_peers=3, n_steps=70, kinds=("text",), styles="rich", snapshots=snaps)
        full = _fuzz.blobs_of(reps)
        for fr, _ in snaps[:: max(1, len(snaps) // 8)]:
            docs.append(list(full)); fronts.append(wire.encode_frontiers(fr))
    r = wire.Replica(77)
    r.text_insert("text", 0, "abcdef"); r.text_mark("text", 1, 4, "bold", True); r.text_insert("text", 0, "Z"); r.commit()
    blob = [r.export()]
    for c in range(0, 9):   # frontiers at every op of the change: between the two anchors as well
        docs.append(list(blob)); fronts.append(wire.encode_frontiers([(77, c)]))
    return docs, fronts


def resident_sessions(seeds, n_steps=5):
    out = []
    for seed in seeds:
        rng = random.Random(seed * 11 + 3)
        snaps = []
        reps = _fuzz.random_session(seed, n_peers=rng.randint(2, 4), n_steps=rng.randint(60, 140), kinds=("text",), snapshots=snaps, styles="rich")
        out.append(_resident.plan_steps(_resident.chunked_blobs(reps, rng), rng, n_steps, versions=[v for v, _ in snaps]))
    return out


def run_resident(ctx, sessions):
    """per step: [(status, richtext bytes)] from lm_richtext behind every lm_run"""
    got = []
    for k in range(len(sessions[0])):
        docs = [s[k][0] for s in sessions]
        fr = [s[k][1] for s in sessions]
        if k == 0:
            ctx.stage(docs, fr)
            ctx.import_more([[] for _ in docs], fr)
        else:
            ctx.import_more(docs, fr)
        ctx.run()
        res = ctx.fetch()
        rt = ctx.richtext()
        got.append([(r[0], t[0], t[1]) for r, t in zip(res, rt)])
    return got


def oracle_resident(sessions):
    out = [[] for _ in sessions[0]]
    for s in sessions:
        o = _oracle.Session()
        o.want_richtext = True
        for k, (blobs, f) in enumerate(s):
            st = o.step(blobs, f)
            out[k].append((st[0], o.richtext()))
        o.close()
    return out


def same(got, want, what=""):
    """got / want: [(status, bytes)].  Equal statuses, equal bytes (members in the bytewise order of their JSON-encoded keys on both sides)"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (what, i, g[0], w[0])
        if w[0] == 0:
            assert g[1] == w[1], (what, i, g[1][:400], w[1][:400])


import functools


@functools.lru_cache(maxsize=None)
def _base_rich():
    return [_fuzz.blobs_of(_fuzz.random_session(9000 + s, n_peers=3, n_steps=80, kinds=("text",), styles="rich")) for s in range(12)]


@functools.lru_cache(maxsize=None)
def _base_mixed():
    base = [_fuzz.blobs_of(_fuzz.random_session(9100 + s, n_peers=3, n_steps=90, kinds=("text", "list", "map"), styles="rich")) for s in range(8)]
    base += [_fuzz.blobs_of(_fuzz.nested_session(9200 + s, n_steps=100)) for s in range(6)]
    base += [_fuzz.blobs_of(_fuzz.movable_session(9300 + s, n_peers=3, n_steps=90, nested=s % 2 == 0)) for s in range(6)]
    return base


def damaged_docs(n=400, seed=5):
    """rich-text sessions (marks of several keys, multi-byte scalars) with one blob damaged by byte flips and the envelope checksum re-fitted"""
    import struct
    rng = random.Random(seed)
    base = _base_rich()

    def refit(blob):
        body = blob[20:]
        return blob[:16] + struct.pack("<I", _oracle.xxh32(body)) + body
    docs = []
    for _ in range(n):
        d = list(rng.choice(base)); j = rng.randrange(len(d)); b = bytearray(d[j])
        for _ in range(rng.choice([1, 1, 2, 4])):
            k = rng.randrange(22, len(b))
            b[k] = rng.choice([b[k] ^ (1 << rng.randrange(8)), rng.randrange(256), 0xFF, 0x80, 0])
        d[j] = refit(bytes(b))
        docs.append(d)
    return docs


def check_damaged(run, docs):
    """run(docs) -> (merge results, richtext results).  What both sides accept is rendered alike (JSON, version vector, richtext), and the
    device never renders a document the oracle rejects.  Returns (both accept, only the oracle accepts)."""
    want, want_j = _oracle.richtext_batch(docs, threads=16, with_merge=True)
    got_j, got = run(docs)
    n_both = n_oracle_only = 0
    for i in range(len(docs)):
        g, w = got_j[i], want_j[i]
        assert not (g[0] == 0 and w[0] not in (0, 4)), (i, "the device rendered a document the oracle rejects", w[0])
        if g[0] == 0 and w[0] == 0:
            n_both += 1
            assert g == w and got[i] == want[i], (i, g[1][:200], w[1][:200])
        n_oracle_only += g[0] != 0 and w[0] == 0
    return n_both, n_oracle_only


def damaged_mixed_docs(n=600, seed=1):
    """rich-text + list + map sessions, nested containers and MovableLists, one blob damaged per document by byte flips, truncation, a
    spliced range or a duplicated range, checksum re-fitted (the corpus that turned up the last-lamport rule, the surplus run in the
    message-length column and the insert beyond the end)"""
    import struct
    rng = random.Random(seed)
    base = _base_mixed()

    def refit(blob):
        body = blob[20:]
        return blob[:16] + struct.pack("<I", _oracle.xxh32(body)) + body

    def corrupt(blob):
        b = bytearray(blob)
        k = rng.random()
        if k < 0.6:
            for _ in range(rng.choice([1, 1, 2, 5])):
                i = rng.randrange(22, len(b))
                b[i] = rng.choice([b[i] ^ (1 << rng.randrange(8)), rng.randrange(256), 0xFF, 0x80, 0])
        elif k < 0.75:
            del b[rng.randrange(22, len(b)):]
        elif k < 0.9:
            i = rng.randrange(22, len(b)); j = min(len(b), i + rng.randrange(1, 40))
            b[i:j] = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 50)))
        else:
            i = rng.randrange(22, len(b))
            b[i:i] = b[rng.randrange(22, len(b)):][: rng.randrange(1, 64)]
        return refit(bytes(b)) if len(b) > 22 else bytes(b)
    docs = []
    for _ in range(n):
        d = list(rng.choice(base)); j = rng.randrange(len(d)); d[j] = corrupt(d[j])
        docs.append(d)
    return docs


# ---------------------------------------------------------------------------------------------------------------------------------
# Spans joined BY VALUE (richtext_state.rs:2546-2584 joins two spans iff their attribute maps are equal LoroValues, value.rs:29-44):
# documents in which whether two neighbouring ranges are one span — and which of the two values the span then shows — is decided by
# the equality of two style values alone.  Checked against tests/_richtext_ref.py, which shares no code with the oracle.
import struct

import _richtext_ref

TEXT = wire.root_cid("t", wire.KIND_TEXT)


class PairMap(dict):
    """a map value whose ENCODED entries are exactly `pairs`, duplicated keys included (written like _cases.nested_map_order_docs
    writes them); as a Python dict it holds what a map built by successive inserts holds: of a duplicated key the last value"""
    def __init__(self, pairs):
        super().__init__(pairs)
        self.pairs = list(pairs)

    def items(self):
        return self.pairs

    def __len__(self):
        return len(self.pairs)


def _f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def value_pairs():
    """[(name, v1, v2, equal)] — `equal` as LoroValue's PartialEq has it.  Every pair is used in both orders: a joined span shows
    the FIRST value."""
    nans = [0x7ff8000000000000, 0x7ff8000000000001, 0xfff8000000000000, 0x7ff0000000000001]
    out = [("nan %x / %x" % (a, b), _f(a), _f(b), True) for i, a in enumerate(nans) for b in nans[i + 1:]]
    nan, nan2, inf = _f(nans[0]), _f(nans[2]), float("inf")
    out += [
        ("0.0 / -0.0", 0.0, -0.0, True),
        ("map key order", {"a": 1, "b": 2}, {"b": 2, "a": 1}, True),
        ("duplicated key / last wins", PairMap([("k", 1), ("a", 2), ("k", 3)]), {"a": 2, "k": 3}, True),
        ("list of zero and map of nan", [0.0, {"x": nan}], [-0.0, {"x": nan2}], True),
        ("nested maps reversed", {"m": {"p": [1, {"q": -0.0}], "o": "s"}, "l": 2}, {"l": 2, "m": {"o": "s", "p": [1, {"q": 0.0}]}}, True),
        ("inf / -inf", inf, -inf, False),
        ("inf / nan", inf, nan, False),
        ("[nan] / [null]", [nan], [None], False),
        ("1 / 1.0", 1, 1.0, False),
        ("true / 1", True, 1, False),
        ("false / 0", False, 0, False),
        ("'1' / 1", "1", 1, False),
        ("'' / b''", "", b"", False),
        ("[1,2] / b'\\1\\2'", [1, 2], b"\x01\x02", False),
        ("[] / {}", [], {}, False),
        ("[1] / [1,1]", [1], [1, 1], False),
        ("{a:1} / {a:1,b:null}", {"a": 1}, {"a": 1, "b": None}, False),
        ("'a' / 'a\\0'", "a", "a\x00", False),
        ("e-acute composed / decomposed", "\u00e9", "e\u0301", False),
        ("i64 min / max", -2 ** 63, 2 ** 63 - 1, False),
        ("2^53+1 / 2^53 as a double", 9007199254740993, 9007199254740992.0, False),
    ]
    for name, a, b, eq in out:
        assert _richtext_ref.value_eq(a, b) == eq and _richtext_ref.value_eq(b, a) == eq, name
    return out


class Writer:
    """one peer writing Text "t": marks are given in SCALAR positions, every commit records (frontiers, the visible order — anchors
    included — at that version)"""
    def __init__(self, peer, text=None):
        self.r = wire.Replica(peer)
        self.anchors = set()
        self.versions = []
        if text is not None:
            self.r.text_insert("t", 0, text)

    def _ents(self):
        return [i for i, e in enumerate(self.r.seq[TEXT]) if e not in self.anchors]

    def mark(self, i, j, key, value):
        """Start anchor in front of scalar i, End anchor behind scalar j - 1"""
        ents = self._ents()
        c0 = self.r.next_counter
        self.r.text_mark("t", ents[i], ents[j - 1] + 1, key, value)
        self.anchors |= {(self.r.peer, c0), (self.r.peer, c0 + 1)}

    def delete(self, i, n):
        """scalars i .. i + n - 1 (no anchor stands between them)"""
        ents = self._ents()
        assert ents[i + n - 1] - ents[i] == n - 1
        self.r.text_delete("t", ents[i], n)

    def commit(self):
        self.r.commit()
        self.versions.append((list(self.r.frontiers), list(self.r.seq[TEXT])))
        return dict(self.r.vv)


class Case:
    """name, the replicas that hold its changes, its blobs — `steps`: the same history as the blobs of successive imports — the visible
    order of Text "t" at the latest version, recorded versions [(frontiers, order)] and the plain reference's bytes"""
    def __init__(self, name, reps, steps, order, versions=()):
        self.name, self.reps, self.steps, self.order, self.versions = name, reps, steps, order, list(versions)
        self.blobs = [b for s in steps for b in s]
        self.changes = _richtext_ref.changes_of(reps)
        self.want = _richtext_ref.richtext_bytes(self.changes, {TEXT: order})

    def want_at(self, k):
        return _richtext_ref.richtext_bytes(self.changes, {TEXT: self.versions[k][1]})


_PEER = [7000]


def _writer(text):
    _PEER[0] += 1
    return Writer(_PEER[0], text)


def _case(name, w, vv1):
    """the writer's history in two imports: everything up to `vv1` (the text and the first marks), then the rest in blocks of its own"""
    return Case(name, [w.r], [[w.r.export()]] if vv1 is None else [[_exp_to(w.r, vv1)], [w.r.export(from_vv=vv1)]], w.r.seq[TEXT], w.versions)


def _exp_to(r, vv):
    own = wire.Replica(r.peer)
    own.changes = {r.peer: [c for c in r.changes[r.peer] if c.ctr_end <= vv[r.peer]]}
    return own.export()


def placements(v1, v2, name=""):
    """[Case] — small single-writer documents (6 to 70 scalars) in which v1 and v2 are the values of key "c" on two neighbouring
    ranges; first commit: the text and the first range's marks, second commit: the rest (a block of its own in `steps`)"""
    out = []

    def doc(what, text, first, second):
        w = _writer(text)
        first(w)
        vv1 = w.commit()
        second(w)
        w.commit()
        out.append(_case("%s: %s" % (name, what), w, vv1))

    doc("touching", "abcdef", lambda w: w.mark(0, 3, "c", v1), lambda w: w.mark(3, 6, "c", v2))
    doc("a deleted run between", "abcXYdef", lambda w: w.mark(0, 3, "c", v1), lambda w: (w.mark(5, 8, "c", v2), w.delete(3, 2)))
    doc("an unmarked scalar between", "abc-def", lambda w: w.mark(0, 3, "c", v1), lambda w: w.mark(4, 7, "c", v2))
    doc("v1 v2 v1", "abcdefghi", lambda w: (w.mark(0, 3, "c", v1), w.mark(6, 9, "c", v1)), lambda w: w.mark(3, 6, "c", v2))
    doc("two keys, the other one equal", "abcdef", lambda w: (w.mark(0, 3, "x", v1), w.mark(0, 3, "y", "same")), lambda w: (w.mark(3, 6, "y", "same"), w.mark(3, 6, "x", v2)))
    doc("two keys, the other one differs", "abcdef", lambda w: (w.mark(0, 3, "x", v1), w.mark(0, 3, "y", "one")), lambda w: (w.mark(3, 6, "y", "two"), w.mark(3, 6, "x", v2)))
    doc("a later mark overrides one side", "abcdef", lambda w: (w.mark(0, 3, "c", v1), w.mark(3, 6, "c", v2)), lambda w: w.mark(3, 6, "c", v1))
    doc("a later mark overrides both sides", "abcdefg", lambda w: (w.mark(0, 3, "c", v1), w.mark(3, 6, "c", v2)), lambda w: (w.mark(0, 2, "c", "w"), w.mark(4, 7, "c", "w")))
    # 70 scalars, the boundary at every position 60..68: the change of attributes on either side of the kernel's 64-element step,
    # an anchor in its last lanes and its first
    text70 = "".join(chr(0x41 + i % 26) for i in range(70))
    for b in range(60, 69):
        doc("boundary at %d" % b, text70, lambda w, b=b: w.mark(0, b, "c", v1), lambda w, b=b: w.mark(b, 70, "c", v2))
    return out


def _block_keys(changes):
    """the key table of the block wire.encode_block writes for `changes`, read back from its bytes: five varints, then the
    length-prefixed sections header, meta, container ids, KEYS, …"""
    b = wire.encode_block(changes)
    at = 0

    def uleb():
        nonlocal at
        v = sh = 0
        while True:
            x = b[at]; at += 1
            v |= (x & 0x7F) << sh; sh += 7
            if not x & 0x80:
                return v
    for _ in range(5):
        uleb()
    for _ in range(3):
        n = uleb(); at += n
    end = uleb() + at
    keys = []
    while at < end:
        n = uleb(); keys.append(b[at:at + n].decode()); at += n
    return keys, b


def _premise(block1, v1, block2, v2, same_key):
    """what the cross-block cases are about, checked on the blocks' own bytes: the two maps' single keys sit at the SAME index of
    their blocks' key tables iff they are different keys, so the encoded values are the same bytes iff the maps differ"""
    (k1, b1), (k2, b2) = _block_keys(block1), _block_keys(block2)
    (key1,), (key2,) = v1.keys(), v2.keys()
    i1, i2 = k1.index(key1), k2.index(key2)
    assert (key1 == key2) == same_key and (i1 == i2) == (not same_key), (k1, k2)
    e1, e2 = b"\x08\x01" + wire.uleb(i1) + b"\x03\x01", b"\x08\x01" + wire.uleb(i2) + b"\x03\x01"     # map of one entry: key index, I64 1
    assert e1 in b1 and e2 in b2 and (e1 == e2) == (not same_key)


def cross_block_cases():
    """[Case] — a nested map's keys are indices into its BLOCK's key table (docs/encoding.md §10.1): {"a":1} and {"b":1} whose
    keys have the same index in two blocks are the same bytes and different maps; {"a":1} twice with "a" at different indices is
    different bytes and the same map.  Each with both marks by one peer (two exports) and by two peers."""
    out = []
    for what, v1, v2, extra in (("same index, different keys", {"a": 1}, {"b": 1}, False), ("different index, same key", {"a": 1}, {"a": 1}, True)):
        for order in (0, 1):
            a, b = (v1, v2) if order == 0 else (v2, v1)
            w = _writer("abcdef")
            w.mark(0, 3, "c", a)
            vv1 = w.commit()
            if extra:
                w.mark(3, 6, "q", None)     # registers another key in front of "c" and "a" in the second block's table
            w.mark(3, 6, "c", b)
            w.commit()
            c = _case("one peer: %s (%d)" % (what, order), w, vv1)
            _premise(w.r.changes[w.r.peer][:1], a, w.r.changes[w.r.peer][1:], b, extra)
            out.append(c)
            # two peers: the second one has imported the first one's change and marks the other half
            w1 = _writer("abcdef")
            w1.mark(0, 3, "c", a)
            w1.commit()
            w2 = _writer(None)
            w2.r.merge_from(w1.r)
            w2.r.set_visible("t", wire.KIND_TEXT, w1.r.seq[TEXT])
            w2.anchors = set(w1.anchors)
            if extra:
                w2.mark(3, 6, "q", None)
            w2.mark(3, 6, "c", b)
            w2.commit()
            own = wire.Replica(w2.r.peer); own.changes = {w2.r.peer: w2.r.changes[w2.r.peer]}
            _premise(w1.r.changes[w1.r.peer], a, w2.r.changes[w2.r.peer], b, extra)
            out.append(Case("two peers: %s (%d)" % (what, order), [w2.r], [[w1.r.export()], [own.export()]], w2.r.seq[TEXT],
                            [w1.versions[0], w2.versions[0]]))
    return out


@functools.lru_cache(maxsize=None)
def value_corpus():
    """every pair in both orders at every placement, and the cross-block cases"""
    out = []
    for name, v1, v2, _ in value_pairs():
        out += placements(v1, v2, name) + placements(v2, v1, name + " (swapped)")
    return out + cross_block_cases()


def table_rows():
    """the six rows measured in the issue that asked for this corpus: (row, [Case]) — "abcdef", abc marked c=v1, def c=v2"""
    nans = (_f(0x7ff8000000000000), _f(0xfff8000000000001))
    rows = [("1 same index, different keys", [c for c in cross_block_cases() if "same index" in c.name])]
    for row, v1, v2 in (("2 map key order", {"a": 1, "b": 2}, {"b": 2, "a": 1}), ("3 two NaNs", nans[0], nans[1]), ("4 0.0 / -0.0", 0.0, -0.0),
                        ("5 inf / -inf", float("inf"), float("-inf")), ("5 inf / nan", float("inf"), nans[0]), ("6 1 / 1.0", 1, 1.0)):
        rows.append((row, placements(v1, v2, row)[:1]))
    return rows


def limit_cases():
    """[(name, Case, renders)] — RT_MAX = 64 (lm_k_richtext.h): 63 / 64 StyleOps open at one scalar on distinct keys render, 65 are
    LM_UNSUPPORTED for that document's rich-text status only; 64 distinct style keys over one Text render, 65 do not; plain
    neighbours between them"""
    out = []

    def plain(name):
        w = _writer("neighbour"); w.mark(2, 5, "bold", True); w.commit()
        out.append((name, _case(name, w, None), True))
    for n in (63, 64, 65):
        w = _writer("ab")
        for k in range(n):
            w.mark(0, 2, "k%02d" % k, k)
        w.commit()
        out.append(("%d open at one scalar" % n, _case("%d open" % n, w, None), n <= 64))
        plain("neighbour behind %d open" % n)
    for n in (64, 65):
        w = _writer("".join(chr(0x30 + i) for i in range(n)))
        for k in range(n):
            w.mark(k, k + 1, "k%02d" % k, k)
        w.commit()
        out.append(("%d distinct keys" % n, _case("%d keys" % n, w, None), n <= 64))
        plain("neighbour behind %d keys" % n)
    return out


def check_cases(got, cases, what=""):
    """got: [(status, bytes)] of lm_richtext for the cases' documents — byte-exact against the plain reference"""
    assert len(got) == len(cases)
    bad = [(c.name, g[0], g[1][:300], c.want[:300]) for g, c in zip(got, cases) if g[0] != 0 or g[1] != c.want]
    assert not bad, (what, len(bad), bad[:4])


def checkout_docs(cases):
    """(cases' index, version index, blobs, encoded frontiers) for every recorded version of every case"""
    return [(i, k, c.blobs, wire.encode_frontiers(c.versions[k][0])) for i, c in enumerate(cases) for k in range(len(c.versions))]


def step_sessions(cases):
    """run_resident() sessions: the first import and its version, then the rest — the second mark arrives in a later import step"""
    two = [c for c in cases if len(c.steps) == 2]
    return two, [[(c.steps[0], None), (c.steps[1], None)] for c in two]
