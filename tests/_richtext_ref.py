"""A PLAIN reference of get_richtext_value's style rule (container/richtext/richtext_state.rs:2500-2584): no oracle, kernel or
decoder code.  It works from the writers' Change / Op objects (loro_amd.wire), so style values are Python objects, and from the
visible element order of each Text, anchors included, which is the integrate stage's job and has tests of its own.

  - a Start anchor opens its StyleOp iff its End anchor (peer, counter + 1) is visible behind it;
  - per key the op with the greatest (lamport, peer) decides, the lamport being the change's plus the op's offset in the change;
  - a None value removes the key;
  - a scalar joins the previous span iff value_eq(previous attributes, attributes) — LoroValue's PartialEq
    (loro-common/src/value.rs:29-44) — and a joined span keeps the previous span's attributes.
"""
import math

from _values import to_json


def _kind(v):
    """the LoroValue variant of a Python value (bool before int: True is not 1; bytes and list are kinds of their own)"""
    if v is None:
        return 0
    if isinstance(v, bool):
        return 1
    if isinstance(v, int):
        return 2
    if isinstance(v, float):
        return 3
    if isinstance(v, str):
        return 4
    if isinstance(v, (bytes, bytearray)):
        return 5
    if isinstance(v, (list, tuple)):
        return 6
    if isinstance(v, dict):
        return 7
    raise TypeError(type(v))


def value_eq(a, b):
    """value.rs:29-44: different kinds are never equal; doubles by == or both NaN; lists elementwise; maps by key set, then per key"""
    k = _kind(a)
    if k != _kind(b):
        return False
    if k == 3:
        return a == b or (math.isnan(a) and math.isnan(b))
    if k == 5:
        return bytes(a) == bytes(b)
    if k == 6:
        return len(a) == len(b) and all(value_eq(x, y) for x, y in zip(a, b))
    if k == 7:
        return set(a.keys()) == set(b.keys()) and all(value_eq(a[key], b[key]) for key in a.keys())
    return a == b


def _index(changes, cid):
    """element id -> ("char", c) | ("start", (lamport, peer, key, value)) | ("end",) for the ops of Text `cid`"""
    what = {}
    for ch in changes:
        for op in ch.ops:
            if op.cid != cid:
                continue
            if op.kind == "text_insert":
                for i, c in enumerate(op.text):
                    what[(ch.peer, op.counter + i)] = ("char", c)
            elif op.kind == "style_start":
                what[(ch.peer, op.counter)] = ("start", (ch.lamport + (op.counter - ch.counter), ch.peer, op.key, op.value))
            elif op.kind == "style_end":
                what[(ch.peer, op.counter)] = ("end",)
    return what


def spans(changes, cid, order):
    """[[attributes dict, text]] of Text `cid` whose visible elements, anchors included, are `order` (ids, in sequence order)"""
    what = _index(changes, cid)
    at = {e: i for i, e in enumerate(order)}
    active, out = {}, []          # active: Start id -> StyleOp
    for i, e in enumerate(order):
        w = what[e]
        if w[0] == "start":
            if at.get((e[0], e[1] + 1), -1) > i:
                active[e] = w[1]
        elif w[0] == "end":
            active.pop((e[0], e[1] - 1), None)
        else:
            best = {}
            for lam, peer, key, value in active.values():
                if key not in best or best[key][:2] < (lam, peer):
                    best[key] = (lam, peer, value)
            attrs = {k: v[2] for k, v in best.items() if v[2] is not None}
            if out and value_eq(out[-1][0], attrs):
                out[-1][1] += w[1]
            else:
                out.append([attrs, w[1]])
    return out


def cid_string(cid):
    return "cid:root-%s:Text" % cid.name if cid.root else "cid:%d@%d:Text" % (cid.counter, cid.peer)


def richtext_bytes(changes, orders):
    """the bytes lm_richtext returns for a document: {"cid:…:Text":[span,…],…} over the Texts of `orders` (cid -> visible ids) in
    which something is visible, canonical JSON (keys in bytewise order; no attributes entry when there are none)"""
    changes = list(changes)
    doc = {}
    for cid, order in orders.items():
        if order:
            doc[cid_string(cid)] = [({"attributes": a, "insert": t} if a else {"insert": t}) for a, t in spans(changes, cid, order)]
    return to_json(doc).encode("utf-8")


def changes_of(reps):
    """every change the replicas hold, once"""
    seen = {}
    for r in reps:
        for chs in r.changes.values():
            for c in chs:
                seen[(c.peer, c.counter)] = c
    return list(seen.values())
