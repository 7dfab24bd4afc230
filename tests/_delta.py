"""Text / List deltas between two versions (lm_delta): the plain reference, from the oracle alone, and the cases shared by the
kernel-logic (CPU) and the GPU tests.

  * ids_A = _oracle.visible_ids(blobs at A), ids_V = _oracle.visible_ids(blobs at V): both are subsequences of ONE sequence order,
    so the common ids in order are the retains and the canonical delta follows by a two-pointer walk — no tracker order is needed;
  * insert payloads are taken from the oracle's own JSON at V (a Text's raw string literal split into one escaped piece per scalar,
    a List's raw array split at its top-level commas): the expected bytes are the oracle's bytes, not a re-serialisation;
  * widths for units == 1 come from the oracle's string at A (deletes, retains);
  * from_vv = the vv bytes _oracle.merge(blobs at A) returns.
A second, form-independent check on every case: applying the returned ops to the oracle's value at A gives the oracle's value at V."""
import json
import random

import _cursor, _fuzz, _oracle
from loro_amd import wire

TEXT, LIST = "cid:root-text:Text", "cid:root-list:List"
ROOTS = (("text", wire.KIND_TEXT, TEXT), ("list", wire.KIND_LIST, LIST))
OK, DECODE_ERROR, UNSUPPORTED, FRONTIERS_NOT_FOUND = 0, 1, 4, 6


# ---- the oracle's JSON, raw
def _skip(s, i):
    """index behind the JSON value that starts at s[i]"""
    if s[i] == '"':
        i += 1
        while s[i] != '"':
            i += 2 if s[i] == "\\" else 1
        return i + 1
    if s[i] in "[{":
        depth = 0
        while True:
            if s[i] == '"':
                i = _skip(s, i)
                continue
            depth += s[i] in "[{"
            depth -= s[i] in "]}"
            i += 1
            if depth == 0:
                return i
    while i < len(s) and s[i] not in ",]}":
        i += 1
    return i


def raw_members(js):
    """{key: raw value text} of a JSON object, values exactly as they stand"""
    s = js.decode() if isinstance(js, bytes) else js
    out, i = {}, 1
    while s[i] != "}":
        e = _skip(s, i)
        key = json.loads(s[i:e])
        v = _skip(s, e + 1)
        out[key] = s[e + 1:v]
        i = v + (s[v] == ",")
    return out


def string_pieces(raw):
    """a raw JSON string literal -> one escaped piece per Unicode scalar (the emitter writes \\u00XX for control characters only)"""
    body, out, i = raw[1:-1], [], 0
    while i < len(body):
        n = 1 if body[i] != "\\" else 6 if body[i + 1] == "u" else 2
        out.append(body[i:i + n])
        i += n
    return out


def array_pieces(raw):
    out, i = [], 1
    while raw[i] != "]":
        e = _skip(raw, i)
        out.append(raw[i:e])
        i = e + (raw[e] == ",")
    return out


# ---- the canonical delta of one container
def canonical(ids_a, w_a, ids_v, pieces_v):
    """[(kind, payload)]: ("retain", n) | ("insert", [pieces]) | ("delete", n); w_a = the widths of A's elements in the asked units"""
    in_a, in_v = set(ids_a), set(ids_v)
    ops, i, j = [], 0, 0
    while i < len(ids_a) or j < len(ids_v):
        dels, ins = 0, []
        while i < len(ids_a) and ids_a[i] not in in_v:
            dels += w_a[i]; i += 1
        while j < len(ids_v) and ids_v[j] not in in_a:
            ins.append(pieces_v[j]); j += 1
        if ins:
            ops.append(("insert", ins))
        if dels:
            ops.append(("delete", dels))
        n = 0
        while i < len(ids_a) and j < len(ids_v) and ids_a[i] == ids_v[j]:
            n += w_a[i]; i += 1; j += 1
        if n:
            ops.append(("retain", n))
        else:
            assert i == len(ids_a) and j == len(ids_v), "the two versions do not share one sequence order"
    if ops and ops[-1][0] == "retain":
        ops.pop()
    return ops


def op_bytes(ops, text):
    out = []
    for k, v in ops:
        if k == "insert":
            out.append('{"insert":"%s"}' % "".join(v) if text else '{"insert":[%s]}' % ",".join(v))
        else:
            out.append('{"%s":%d}' % (k, v))
    return "[" + ",".join(out) + "]"


def _width(ch, units):
    return 2 if units == 1 and ord(ch) >= 0x10000 else 1


class At:
    """the oracle's view of the root containers of a document at one version"""

    def __init__(self, blobs, ids=None):
        """blobs = updates that hold exactly the version's causal history ([] = the empty version); ids = {root name: visible ids}
        from another source than the oracle (the plain merge model, _merge_ref.py)"""
        self.blobs = list(blobs)
        if blobs:
            st, js, vv, _ = _oracle.merge(blobs)
            assert st == 0
        else:
            js, vv = b"{}", None
        self.vv, self.raw, self.value = vv, raw_members(js), json.loads(js)
        self.ids = {name: (_oracle.visible_ids(blobs, name, kind) if blobs else []) for name, kind, _ in ROOTS} if ids is None else ids


def expected(a, v, units=0):
    """(bytes, {cid: ops}) lm_delta must give from version `a` to version `v` for the root containers text / list"""
    members, all_ops = {}, {}
    for name, kind, cid in ROOTS:
        text = kind == wire.KIND_TEXT
        va, vv_ = a.value.get(name, "" if text else []), v.value.get(name, "" if text else [])
        if text:
            pieces = string_pieces(v.raw.get(name, '""'))
            w_a = [_width(ch, units) for ch in va]
        else:
            pieces = array_pieces(v.raw.get(name, "[]"))
            w_a = [1] * len(va)
        assert len(pieces) == len(v.ids[name]) == len(vv_) and len(va) == len(a.ids[name]), (name, len(pieces), len(v.ids[name]))
        ops = canonical(a.ids[name], w_a, v.ids[name], pieces)
        all_ops[cid] = ops
        if ops:
            members[cid] = op_bytes(ops, text)
    body = ",".join('"%s":%s' % (k, members[k]) for k in sorted(members, key=lambda k: json.dumps(k).encode()))
    return ("{" + body + "}").encode(), all_ops


def apply(value, ops, units=0):
    """the ~20-line applier: ops on the scalar list of a string / the element list -> the new value (form-independent check)"""
    text = isinstance(value, str)
    src, out, i = list(value), [], 0

    def take(n):   # n units -> that many elements
        nonlocal i
        k = i
        while n > 0:
            n -= _width(src[k], units) if text else 1
            k += 1
        assert n == 0, "a count splits a surrogate pair"
        got, i = src[i:k], k
        return got
    for op in ops:
        if "retain" in op:
            out += take(op["retain"])
        elif "delete" in op:
            take(op["delete"])
        else:
            out += list(op["insert"])
    out += src[i:]
    return "".join(out) if text else out


def check_one(got, a, v, units=0, what=""):
    """one result (status, other_changed, bytes) against the reference: the bytes, then the applier"""
    want, _ = expected(a, v, units)
    assert got[0] == OK, (what, got)
    assert got[2] == want, (what, got[2], want)
    d = json.loads(got[2])
    for name, kind, cid in ROOTS:
        empty = "" if kind == wire.KIND_TEXT else []
        assert apply(a.value.get(name, empty), d.get(cid, []), units) == v.value.get(name, empty), (what, cid)
    return d


def kinds_of(ops):
    return {k for o in ops.values() for k, _ in o}


# ---- fuzz: unstyled Text + List sessions, A = every recorded snapshot version plus the empty version, V = latest
def fuzz_corpus(seeds, n_steps=80, model=False):
    """(docs, [(doc, At(A), At(V))]); model: the writers' views and the ids of every At come from the plain merge model
    (_merge_ref.py) instead of the oracle"""
    docs, pairs = [], []
    for seed in seeds:
        snaps = []
        if model:
            import _merge_ref, _richtext_ref
            reps = _fuzz.random_session(seed, n_peers=3, n_steps=n_steps, kinds=("text", "list"), snapshots=snaps, view=_merge_ref.view)
            m = _merge_ref.Model(_richtext_ref.changes_of(reps))
            ids = lambda fr: {name: m.visible_ids(wire.root_cid(name, kind), fr) for name, kind, _ in ROOTS}
        else:
            reps = _fuzz.random_session(seed, n_peers=3, n_steps=n_steps, kinds=("text", "list"), snapshots=snaps)
            ids = lambda fr: None
        blobs = _fuzz.blobs_of(reps)
        v = At(blobs, ids(None))
        docs.append(blobs)
        pairs.append((len(docs) - 1, At([], ids([])), v))
        for fr, upd in snaps:
            pairs.append((len(docs) - 1, At([upd], ids(fr)), v))
    return docs, pairs


def fuzz_condition(pairs):
    """asserted from the reference alone: at least half of the (document, A) pairs have a delta holding all three op kinds"""
    full = sum(1 for _, a, v in pairs if kinds_of(expected(a, v)[1]) == {"retain", "insert", "delete"})
    assert 2 * full >= len(pairs), (full, len(pairs))
    assert any(expected(a, v)[0] != b"{}" for _, a, v in pairs)


def run_fuzz(ctx, docs, pairs, what=""):
    res = ctx.merge_batch(docs)
    assert res == _oracle.merge_batch(docs, threads=8)
    for units in (0, 1):
        got = ctx.delta([(d, a.vv) for d, a, _ in pairs], units)
        for (d, a, v), g in zip(pairs, got):
            check_one(g, a, v, units, (what, d, units))
            assert g[1] == 0
    assert ctx.fetch() == res
    return len(pairs)


# ---- hand cases: (name, blobs of the document, blobs at A or None, {units: expected bytes}, other_changed)
def _same_ops_two_commits(peer, setup, first, rest):
    """two replicas of ONE peer doing the same edits: the first stops after `first`, the second goes on — the second's delete row is
    cut by the first's version"""
    r1, r2 = wire.Replica(peer), wire.Replica(peer)
    for r in (r1, r2):
        setup(r); r.commit(); first(r)
    rest(r2)
    r1.commit(); r2.commit()
    return [r2.export()], [r1.export()]


def hand_cases():
    out = []
    r = wire.Replica(5); r.text_insert("text", 0, "hello"); r.commit()
    b = [r.export()]
    out.append(("A = V", b, b, {0: b"{}", 1: b"{}"}, 0))
    out.append(("A = empty", b, None, {0: b'{"cid:root-text:Text":[{"insert":"hello"}]}'}, 0))
    r = wire.Replica(6); r.text_insert("text", 0, "abc"); r.commit(); a = [r.export()]
    r.text_delete("text", 0, 3); r.commit()
    out.append(("everything deleted", [r.export()], a, {0: b'{"cid:root-text:Text":[{"delete":3}]}'}, 0))
    r = wire.Replica(7); r.text_insert("text", 0, "ab"); r.text_delete("text", 0, 2); r.commit(); a = [r.export()]
    r.list_insert("list", 0, [1]); r.commit()
    out.append(("an empty container", [r.export()], a, {0: b'{"cid:root-list:List":[{"insert":[1]}]}'}, 0))
    r = wire.Replica(8); r.text_insert("text", 0, "abcd"); r.commit(); a = [r.export()]
    r.text_delete("text", 1, 1); r.text_insert("text", 1, "X"); r.text_delete("text", 2, 1); r.commit()      # a [b] X [c] d
    out.append(("interleaved gap", [r.export()], a, {0: b'{"cid:root-text:Text":[{"retain":1},{"insert":"X"},{"delete":2}]}'}, 0))
    r = wire.Replica(9); r.text_insert("text", 0, "a\U0001F600b\U0001F600c"); r.commit(); a = [r.export()]
    r.text_insert("text", 2, "X"); r.text_delete("text", 4, 1); r.commit()                                   # "a😀Xbc"
    out.append(("astral", [r.export()], a, {0: b'{"cid:root-text:Text":[{"retain":2},{"insert":"X"},{"retain":1},{"delete":1}]}',
                                            1: b'{"cid:root-text:Text":[{"retain":3},{"insert":"X"},{"retain":1},{"delete":2}]}'}, 0))
    r = wire.Replica(10); r.text_insert("text", 0, "a"); r.commit(); a = [r.export()]
    r.text_insert("text", 1, "\"\\\n\x01"); r.commit()
    out.append(("escapes", [r.export()], a, {0: b'{"cid:root-text:Text":[{"retain":1},{"insert":"\\"\\\\\\n\\u0001"}]}'}, 0))
    # a forward run and a backspace run of 5 deletes, each cut by A after 2 atoms
    v, a = _same_ops_two_commits(11, lambda r: r.text_insert("text", 0, "abcdefgh"), lambda r: r.text_delete("text", 1, 2),
                                 lambda r: r.text_delete("text", 1, 3))
    out.append(("forward run cut by A", v, a, {0: b'{"cid:root-text:Text":[{"retain":1},{"delete":3}]}'}, 0))

    def back(r, n, p0):
        for k in range(n):
            r.text_delete("text", p0 - k, 1)
    v, a = _same_ops_two_commits(12, lambda r: r.text_insert("text", 0, "abcdefgh"), lambda r: back(r, 2, 6), lambda r: back(r, 3, 4))
    out.append(("backspace run cut by A", v, a, {0: b'{"cid:root-text:Text":[{"retain":2},{"delete":3}]}'}, 0))
    # styled: a S b c E d -> anchors never count; the deleted anchor S is no delete (only b is)
    r = wire.Replica(13); r.text_insert("text", 0, "abcd"); r.text_mark("text", 1, 3, "bold", True); r.commit(); a = [r.export()]
    r.text_delete("text", 1, 2); r.text_insert("text", 4, "Z"); r.commit()          # entities a c E d -> a c E d Z
    out.append(("styled", [r.export()], a, {0: b'{"cid:root-text:Text":[{"retain":1},{"delete":1},{"retain":2},{"insert":"Z"}]}'}, 0))
    # a child Text inside a Map created after A; a List insert of a child container; Map writes in V \ A and below A
    r = wire.Replica(14); r.text_insert("text", 0, "t"); r.commit(); a = [r.export()]
    child = r.map_set_container("m", "k", wire.KIND_TEXT); r.text_insert(child, 0, "hey"); r.commit()
    key = b'"cid:%d@14:Text"' % child.counter
    out.append(("child text", [r.export()], a, {0: b"{" + key + b':[{"insert":"hey"}]}'}, 1))
    a2 = [r.export()]
    r.text_insert("text", 1, "u"); r.commit()
    out.append(("map write below A", [r.export()], a2, {0: b'{"cid:root-text:Text":[{"retain":1},{"insert":"u"}]}'}, 0))
    r = wire.Replica(15); r.list_insert("list", 0, [1]); r.commit(); a = [r.export()]
    lc = r.list_insert_container("list", 1, wire.KIND_TEXT); r.text_insert(lc, 0, "in"); r.commit()
    want = ('{"cid:%d@15:Text":[{"insert":"in"}],"cid:root-list:List":[{"retain":1},{"insert":["\U0001F99C:cid:%d@15:Text"]}]}' % (lc.counter, lc.counter)).encode()
    out.append(("list child", [r.export()], a, {0: want}, 0))
    r = wire.Replica(16); r.text_insert("text", 0, "x"); r.commit(); a = [r.export()]
    r.mlist_insert("ml", 0, [1, 2]); r.text_insert("text", 1, "y"); r.commit()
    out.append(("movable list next to a text", [r.export()], a, {0: b'{"cid:root-text:Text":[{"retain":1},{"insert":"y"}]}'}, 1))
    return out


def run_hand_cases(ctx):
    cases = hand_cases()
    docs = [c[1] for c in cases]
    bad = [docs[0][0][:-2] + b"\x00\x01"]            # a document whose import fails, next to healthy ones
    docs.append(bad)
    res = ctx.merge_batch(docs)
    assert res == _oracle.merge_batch(docs) and res[-1][0] != 0
    for units in (0, 1):
        qs, want = [], []
        for d, (name, _, a_blobs, exp, oc) in enumerate(cases):
            qs.append((d, None if a_blobs is None else _oracle.merge(a_blobs)[2]))
            want.append((OK, oc, exp.get(units, exp[0])))
        got = ctx.delta(qs, units)
        for c, g, w in zip(cases, got, want):
            assert g == w, (c[0], units, g, w)
    # … and the hand-written bytes agree with the derived reference wherever it applies (root text / list, unstyled)
    for d, (name, blobs, a_blobs, exp, _) in enumerate(cases):
        if name in ("styled", "child text", "list child"):
            continue
        for units, e in exp.items():
            assert expected(At(a_blobs or []), At(blobs), units)[0] == e, name
    # statuses
    f = len(docs) - 1
    vv0 = res[0][2]
    peer, ctr = next(iter(_cursor.decode_vv(vv0).items()))

    def enc(d):
        return wire.encode_vv(d)
    got = ctx.delta([(f, None), (0, enc({peer: ctr + 1})), (0, enc({peer: ctr, 424242: 1})), (0, enc({peer: ctr, 424242: 0})), (0, vv0[:-1]), (0, vv0 + b"\x00")])
    assert got[0][0] == res[-1][0] and got[0][2] == b""
    assert [g[0] for g in got[1:]] == [FRONTIERS_NOT_FOUND, FRONTIERS_NOT_FOUND, OK, DECODE_ERROR, DECODE_ERROR], got
    assert got[3][2] == b"{}"
    assert ctx.fetch() == res
    for bad_call in (lambda: ctx.delta([(len(docs), None)]), lambda: ctx.delta([(0, None)], units=2)):
        try:
            bad_call()
        except RuntimeError:
            continue
        raise AssertionError("a call that cannot be answered must return -1")
    assert ctx.fetch() == res


# ---- shapes
def chain_halves(n_ops, seed=3):
    """_cursor.chain_case's writer, exported after the first half of its commits and at the end"""
    rng = random.Random(seed)
    r = wire.Replica(21)
    half = None
    for k in range(n_ops):
        ids = r.seq.setdefault(wire.root_cid("text", wire.KIND_TEXT), [])
        if ids and rng.random() < 0.3:
            pos = rng.randrange(len(ids))
            r.text_delete("text", pos, min(len(ids) - pos, rng.randint(1, 3)))
        else:
            r.text_insert("text", rng.randint(0, len(ids)), rng.choice(["a", "bc", "\U0001F600", "déf"]))
        if rng.random() < 0.2:
            r.commit()
        if k == n_ops // 2:
            r.commit()
            half = [r.export()]
    r.commit()
    return half, [r.export()]


def run_chain(ctx, n_ops):
    half, full = chain_halves(n_ops)
    a, v = At(half), At(full)
    _, ops = expected(a, v)
    assert sum(n for k, n in ops[TEXT] if k == "delete") > n_ops // 40        # deletes of prefix content must appear in the delta
    res = ctx.merge_batch([full])
    assert res == _oracle.merge_batch([full])
    for units in (0, 1):
        check_one(ctx.delta([(0, a.vv)], units)[0], a, v, units, "chain")
    check_one(ctx.delta([(0, None)])[0], At([]), v, 0, "chain from the empty version")
    assert ctx.fetch() == res


def long_text(n_chars=6000, seed=9):
    """a Text of more than 64 leaves, three versions; between the last two a gap (interleaved deletes and inserts, 300 elements) that
    spans leaf and 64-element chunk boundaries"""
    rng = random.Random(seed)
    r = wire.Replica(31)
    for k in range(n_chars // 4):
        r.text_insert("text", rng.randint(0, len(r.seq.get(wire.root_cid("text", wire.KIND_TEXT), []))), rng.choice(["abcd", "wxyz", "\U0001F600é!?"]))
        if k % 50 == 0:
            r.commit()
    r.commit(); v1 = [r.export()]
    for _ in range(200):
        ids = r.seq[wire.root_cid("text", wire.KIND_TEXT)]
        r.text_delete("text", rng.randrange(len(ids) - 3), 2)
    r.commit(); v2 = [r.export()]
    for k in range(100):                                                    # one gap: delete 2, insert 1, again and again at one place
        r.text_delete("text", 1000 + k, 2); r.text_insert("text", 1000 + k, "G")
    r.commit()
    return v1, v2, [r.export()]


def run_long_text(ctx):
    v1, v2, v3 = long_text()
    small = [_fuzz.blobs_of(_fuzz.random_session(500 + s, n_peers=3, n_steps=40, kinds=("text", "list"))) for s in range(15)]
    docs = [v3 if d == 7 else small[d if d < 7 else d - 1] for d in range(16)]                 # every seventh document has queries
    res = ctx.merge_batch(docs)
    assert res == _oracle.merge_batch(docs, threads=8)
    v = At(v3)
    _, ops = expected(At(v2), v)
    assert ops[TEXT] == [("retain", ops[TEXT][0][1]), ("insert", ["G"] * 100), ("delete", 200)]
    vs = [At(v1), At(v2), v, At([])]
    q = [(7, a.vv) for a in vs] + [(0, None), (14, None)]                                       # three versions of one document in one call
    for units in (0, 1):
        got = ctx.delta(q, units)
        for a, g in zip(vs, got):
            check_one(g, a, v, units, "long text")
        check_one(got[4], At([]), At(docs[0]), units, "neighbour")
        check_one(got[5], At([]), At(docs[14]), units, "neighbour")
    assert ctx.fetch() == res


def steps(seed=5):
    """a single-writer history exported at three versions: (export, frontiers) each"""
    rng = random.Random(seed)
    r = wire.Replica(31)
    out = []
    for _ in range(3):
        for _ in range(50):
            ids = r.seq.setdefault(wire.root_cid("text", wire.KIND_TEXT), [])
            if ids and rng.random() < 0.35:
                pos = rng.randrange(len(ids))
                r.text_delete("text", pos, min(len(ids) - pos, rng.randint(1, 4)))
            else:
                r.text_insert("text", rng.randint(0, len(ids)), rng.choice(["ab", "c", "\U0001F600d", "xyz"]))
            if rng.random() < 0.3:
                r.commit()
        r.commit()
        out.append((r.export(), list(r.frontiers)))
    return out


def overflow_case(n=4000):
    r = wire.Replica(41)
    r.text_insert("text", 0, "".join(chr(97 + k % 26) for k in range(n))); r.commit()
    a = [r.export()]
    for k in range(n // 2):
        r.text_delete("text", k, 1)                                         # every second character
    r.commit()
    return a, [r.export()]


def run_overflow(ctx):
    a_b, v_b = overflow_case()
    a, v = At(a_b), At(v_b)
    want, _ = expected(a, v)
    assert len(want) > 20 * len(v.raw["text"])                              # ≈ 25 bytes per 2 characters against 1 byte per character
    ctx.set_profiling(1)
    res = ctx.merge_batch([v_b])
    check_one(ctx.delta([(0, a.vv)])[0], a, v, 0, "slab overflow")
    assert ctx.b.delta_bytes(ctx.h) == ((len(want) + 15) & ~15) + 2 * 16                 # the bytes written + a result row per launch
    assert [n for n, _ in ctx.kernel_times()].count("k_delta") == 2        # the second launch, at exact sizes
    ctx.set_profiling(0)
    assert ctx.fetch() == res


def resident_flow(ctx, seeds, n=120):
    """stage + run, keep vv1 from fetch(); import_more + run, delta(from vv1); a third step with A = vv1 again (two imports back)"""
    firsts, seconds, thirds = [], [], []
    for s in seeds:
        f, sec = _cursor.resident_pair(s, n=n)
        firsts.append(f); seconds.append(sec)
        w = wire.Replica(5000 + s)                                          # a third writer, concurrent with everything
        w.text_insert("text", 0, "third"); w.list_insert("list", 0, [s, "x"]); w.commit()
        thirds.append([w.export()])
    ctx.stage(firsts); ctx.run()
    r1 = ctx.fetch()
    vv1 = [r[2] for r in r1]
    a = [At(f) for f in firsts]
    assert [x.vv for x in a] == vv1
    ctx.import_more(seconds); ctx.run()
    r2 = ctx.fetch()
    v2 = [At(f + s) for f, s in zip(firsts, seconds)]
    for units in (0, 1):
        got = ctx.delta([(d, vv1[d]) for d in range(len(seeds))], units)
        for d, g in enumerate(got):
            check_one(g, a[d], v2[d], units, ("resident", d))
    assert ctx.fetch() == r2
    ctx.import_more(thirds); ctx.run()
    r3 = ctx.fetch()
    v3 = [At(f + s + t) for f, s, t in zip(firsts, seconds, thirds)]
    got = ctx.delta([(d, vv1[d]) for d in range(len(seeds))] + [(d, r2[d][2]) for d in range(len(seeds))])
    n = len(seeds)
    for d in range(n):
        check_one(got[d], a[d], v3[d], 0, ("resident, two imports back", d))
        check_one(got[n + d], v2[d], v3[d], 0, ("resident, one import back", d))
    assert ctx.fetch() == r3


def run_bytes_moved(ctx):
    """what crosses to the host is proportional to the change, not to the documents: 40 documents of 20,000 characters, one character
    typed into each — the call copies back the packed answers (each rounded up to 16 bytes) and 16 bytes of result row per query"""
    docs, a_vv, want = [], [], []
    for d in range(40):
        r = wire.Replica(700 + d)
        r.text_insert("text", 0, "".join(chr(97 + (k + d) % 26) for k in range(20000))); r.commit()
        a = At([r.export()])
        r.text_insert("text", 10000 + d, "!"); r.commit()
        docs.append([r.export()]); a_vv.append(a.vv)
        want.append(b'{"cid:root-text:Text":[{"retain":%d},{"insert":"!"}]}' % (10000 + d))
    res = ctx.merge_batch(docs)
    assert sum(len(r[1]) for r in res) > 800000
    got = ctx.delta([(d, a_vv[d]) for d in range(40)])
    assert got == [(OK, 0, w) for w in want]
    assert ctx.b.delta_bytes(ctx.h) == sum((len(w) + 15) & ~15 for w in want) + 40 * 16 < 5000
    assert ctx.fetch() == res


def run_self_check(ctx, monkeypatch):
    """the self-check is the call's safety argument: with LM_DELTA_SKEW the device is handed a V that is one counter short for every
    peer, so "visible by status" disagrees with "c < V[p] and not deleted by an id in V" — through a last op that is an insert (an
    element beyond V is visible) and through one that is a delete (a tombstone whose delete lies beyond V) — and every query must come
    back LM_UNSUPPORTED with no bytes; without the knob the same queries are answered"""
    r = wire.Replica(61); r.text_insert("text", 0, "abcdef"); r.commit(); a1 = At([r.export()])
    r.text_insert("text", 6, "g"); r.commit(); ins = [r.export()]
    r.text_delete("text", 2, 1); r.commit(); dele = [r.export()]
    docs = [ins, dele] + [_fuzz.blobs_of(_fuzz.random_session(800 + s, n_peers=3, n_steps=40, kinds=("text", "list"))) for s in range(4)]
    res = ctx.merge_batch(docs)
    q = [(0, a1.vv), (1, a1.vv)] + [(d, None) for d in range(len(docs))]
    good = ctx.delta(q)
    assert all(g[0] == OK and g[2] != b"{}" for g in good)
    monkeypatch.setenv("LM_DELTA_SKEW", "1")
    assert ctx.delta(q) == [(UNSUPPORTED, 0, b"")] * len(q)
    monkeypatch.delenv("LM_DELTA_SKEW")
    assert ctx.delta(q) == good and ctx.fetch() == res
