"""Stable cursors (lm_cursor_pos / lm_cursor_at): the expected answers, from the oracle alone, and the cases shared by the
kernel-logic (CPU) and the GPU tests.

  * lo_dump_spans gives the spans of a root sequence container over the FULL history in sequence order — an order that does not
    depend on the version;
  * _oracle.visible_ids(blobs at V) gives the ids visible at version V, the oracle's version vector of those blobs says which ids
    V contains;
  * the position of an id at V = the number of ids in front of it in sequence order that are visible at V; its status = OK when it is
    visible, DELETED when V contains it, ID_NOT_FOUND otherwise.
For child containers only the visible ids are at hand (lo_visible_ids2): OK, ID_NOT_FOUND and lm_cursor_at queries only.
The oracle does not say which ids of a styled Text are anchors: the fuzz corpus is unstyled Text + List, styled Text is covered by
hand-built cases whose positions are written out."""
import ctypes
import json
import random

import numpy as np

import _fuzz, _oracle
from loro_amd import wire
from loro_amd._cabi import CURSOR_OK as OK, CURSOR_DELETED as DELETED, CURSOR_ID_NOT_FOUND as NOT_FOUND, \
    CURSOR_CONTAINER_NOT_FOUND as NO_CONTAINER, CURSOR_DOC_FAILED as DOC_FAILED, CURSOR_UNSUPPORTED as UNSUPPORTED

LEFT, MIDDLE, RIGHT = -1, 0, 1
TEXT, LIST = "cid:root-text:Text", "cid:root-list:List"


def spans(blobs, name, kind):
    """[(peer, counter, len)] of root container `name` over the whole history, in sequence order (oracle/lo_capi.cpp lo_dump_spans)"""
    L = _oracle.lib()
    L.lo_dump_spans.restype = ctypes.c_int64
    L.lo_dump_spans.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
    data, off, _ = _oracle.pack([list(blobs)])
    cap = 1 << 16
    while True:
        out = np.zeros(cap * 9, dtype=np.int64)
        n = L.lo_dump_spans(data.ctypes.data, off.ctypes.data, len(blobs), name.encode(), kind, out.ctypes.data, cap)
        assert n >= 0
        if n <= cap:
            break
        cap = int(n)
    return [(int(out[9 * i]), int(out[9 * i + 1]), int(out[9 * i + 2])) for i in range(n)]


def sequence_ids(blobs, name, kind):
    return [(p, c + k) for p, c, ln in spans(blobs, name, kind) for k in range(ln)]


def decode_vv(b):
    def uleb(at):
        v = s = 0
        while True:
            x = b[at]; at += 1
            v |= (x & 0x7f) << s; s += 7
            if x < 0x80:
                return v, at
    n, at = uleb(0)
    vv = {}
    for _ in range(n):
        p, at = uleb(at)
        z, at = uleb(at)
        vv[p] = (z >> 1) ^ -(z & 1)
    return vv


def utf16(s, pos):
    return sum(2 if ord(ch) >= 0x10000 else 1 for ch in s[:pos])


class Expect:
    """the oracle's view of one root sequence container of a document at one version"""

    def __init__(self, all_blobs, at_blobs, name, kind, frontiers=None, model=None):
        """model: a _merge_ref.Model of all_blobs' changes — the sequence order and the visible ids are taken from it, not from the oracle
        (at_blobs must then be all_blobs)"""
        self.order = sequence_ids(all_blobs, name, kind) if model is None else model.sequence_ids(wire.root_cid(name, kind))
        st, js, vv, _ = _oracle.merge(at_blobs, frontiers)
        assert st == 0
        self.vv = decode_vv(vv)
        if model is not None:
            assert frontiers is None and at_blobs is all_blobs
            self.visible = model.visible_ids(wire.root_cid(name, kind))
        elif frontiers is None:
            self.visible = _oracle.visible_ids(at_blobs, name, kind)
        else:   # (single-writer histories only: the version is a prefix of the blobs)
            raise NotImplementedError
        self.vis = set(self.visible)
        self.index = {i: k for k, i in enumerate(self.order)}
        self.vis_index = {i: k for k, i in enumerate(self.visible)}
        self.before, n = [], 0                      # visible ids in front of order[k]
        for i in self.order:
            self.before.append(n); n += i in self.vis
        v = json.loads(js).get(name)
        self.string = v if kind == wire.KIND_TEXT else None
        self.length = len(v) if v is not None else 0
        assert self.length == len(self.visible), (self.length, len(self.visible))
        # the visible ids in sequence order are exactly visible_ids
        assert [i for i in self.order if i in self.vis] == self.visible

    def u16(self, pos):
        if self.string is None:
            return pos
        if not hasattr(self, "_u16"):
            self._u16 = [0]
            for ch in self.string:
                self._u16.append(self._u16[-1] + (2 if ord(ch) >= 0x10000 else 1))
        return self._u16[pos]

    def pos_answer(self, id_, side):
        """(status, pos, pos_utf16, side) lm_cursor_pos must give for `id_`"""
        if id_ is None:
            pos = 0 if side == LEFT else self.length
            return (OK, pos, self.u16(pos), side)
        if id_ in self.vis:
            pos = self.vis_index[id_]
            return (OK, pos, self.u16(pos), side)
        if id_[1] >= 0 and id_[1] < self.vv.get(id_[0], 0) and id_ in self.index:
            pos = self.before[self.index[id_]]
            return (DELETED, pos, self.u16(pos), LEFT)
        return (NOT_FOUND, 0, 0, side)

    def at_answer(self, pos, side):
        """(status, id, side, origin_pos) lm_cursor_at must give (handler.rs:2704-2733)"""
        if self.length == 0:
            return (OK, None, LEFT if side == MIDDLE else side, 0)
        if pos >= self.length:
            return (OK, None, RIGHT, self.length)
        return (OK, self.visible[pos], side, pos)


def container_queries(doc, cid, ex, rng, other_ids=()):
    """every query the issue lists for one container: (pos queries, expected), (at queries, expected)"""
    pq, aq = [], []
    for i, id_ in enumerate(ex.order):              # every visible id, every tombstone (and ids V does not contain yet)
        pq.append((doc, cid, id_, (LEFT, MIDDLE, RIGHT)[i % 3]))
    peers = sorted({p for p, _ in ex.order}) or [7]
    for p in peers:                                 # beyond the version vector
        pq.append((doc, cid, (p, ex.vv.get(p, 0)), MIDDLE))
        pq.append((doc, cid, (p, ex.vv.get(p, 0) + 1000), LEFT))
    pq.append((doc, cid, (peers[-1] + 12345, 0), RIGHT))          # an unknown peer
    pq.append((doc, cid, (peers[0], -1), MIDDLE))
    for id_ in list(other_ids)[:3]:                 # ids of the other container
        pq.append((doc, cid, id_, MIDDLE))
    for side in (LEFT, MIDDLE, RIGHT):
        pq.append((doc, cid, None, side))
    for pos in list(range(ex.length)) + [ex.length, ex.length + 3]:
        aq.append((doc, cid, pos, (MIDDLE, LEFT, RIGHT)[pos % 3]))
    for side in (LEFT, MIDDLE, RIGHT):
        aq.append((doc, cid, ex.length, side))
    return (pq, [ex.pos_answer(q[2], q[3]) for q in pq]), (aq, [ex.at_answer(q[2], q[3]) for q in aq])


def fuzz_session(seed, **kw):
    return _fuzz.random_session(seed, n_peers=kw.pop("n_peers", 3), n_steps=kw.pop("n_steps", 80), kinds=("text", "list"), **kw)


def fuzz_corpus(seeds, model=False, **kw):
    """(docs, pos queries, expected, at queries, expected) over unstyled Text + List sessions; model: the writers' views, the sequence
    order and the visible ids come from the plain merge model (_merge_ref.py) instead of the oracle"""
    docs, pq, pw, aq, aw = [], [], [], [], []
    for seed in seeds:
        m = None
        if model:
            import _merge_ref, _richtext_ref
            reps = fuzz_session(seed, view=_merge_ref.view, **dict(kw))
            m = _merge_ref.Model(_richtext_ref.changes_of(reps))
        else:
            reps = fuzz_session(seed, **dict(kw))
        blobs = _fuzz.blobs_of(reps)
        d = len(docs)
        docs.append(blobs)
        rng = random.Random(seed)
        et, el = Expect(blobs, blobs, "text", wire.KIND_TEXT, model=m), Expect(blobs, blobs, "list", wire.KIND_LIST, model=m)
        for cid, ex, other in ((TEXT, et, el.order), (LIST, el, et.order)):
            (q, w), (q2, w2) = container_queries(d, cid, ex, rng, other)
            pq += q; pw += w; aq += q2; aw += w2
    return docs, pq, pw, aq, aw


def check(ctx, pq, pw, aq, aw, what=""):
    """every query is compared, status included; then the round trip cursor_pos(cursor_at(p)) == p"""
    got = ctx.cursor_pos(pq)
    assert len(got) == len(pw)
    for q, g, w in zip(pq, got, pw):
        assert g == w, (what, "cursor_pos", q, g, w)
    got = ctx.cursor_at(aq)
    assert len(got) == len(aw)
    for q, g, w in zip(aq, got, aw):
        assert g == w, (what, "cursor_at", q, g, w)
    back = [(q[0], q[1], g[1], g[2]) for q, g in zip(aq, got) if g[0] == OK]
    want = [g[3] for g in got if g[0] == OK]
    res = ctx.cursor_pos(back)
    for q, r, w in zip(back, res, want):
        assert r[0] == OK and r[1] == w and r[3] == q[3], (what, "round trip", q, r, w)
    return len(pq) + len(aq) + len(back)


# ---- hand-built cases: (name, blobs, pos queries, expected, at queries, expected); document index 0 in every query
def hand_cases():
    out = []
    # styled text: a S b c E d, then X typed inside, L and R at the edges: entities  a L S b X c E R d  (anchors S = (7,4), E = (7,5))
    t = wire.Replica(7)
    t.text_insert("text", 0, "abcd"); t.text_mark("text", 1, 3, "bold", True); t.commit()
    t.text_insert("text", 3, "X"); t.text_insert("text", 1, "L"); t.text_insert("text", 7, "R"); t.commit()
    # ids: a0 b1 c2 d3 S4 E5 X6 L7 R8; text "aLbXcRd"
    pq = [(0, TEXT, (7, c), MIDDLE) for c in range(9)]
    pw = [(OK, 0, 0, 0), (OK, 2, 2, 0), (OK, 4, 4, 0), (OK, 6, 6, 0), (OK, 2, 2, 0), (OK, 5, 5, 0), (OK, 3, 3, 0), (OK, 1, 1, 0), (OK, 5, 5, 0)]
    aq = [(0, TEXT, p, RIGHT) for p in range(9)]
    aw = [(OK, (7, c), RIGHT, p) for p, c in enumerate([0, 7, 1, 6, 2, 8, 3])] + [(OK, None, RIGHT, 7)] * 2
    out.append(("styled text", [t.export()], pq, pw, aq, aw))
    # a deleted anchor, a deleted scalar behind an anchor: a S b c E d -> delete entity 1 (S) and entity 2 (b)
    u = wire.Replica(8)
    u.text_insert("text", 0, "abcd"); u.text_mark("text", 1, 3, "bold", True); u.commit()
    u.text_delete("text", 1, 2); u.commit()          # ids a0 b1 c2 d3 S4 E5, deletes are ops 6..7; entities now a c E d
    pq = [(0, TEXT, (8, c), RIGHT) for c in range(8)]
    pw = [(OK, 0, 0, 1), (DELETED, 1, 1, -1), (OK, 1, 1, 1), (OK, 2, 2, 1), (DELETED, 1, 1, -1), (OK, 2, 2, 1), (NOT_FOUND, 0, 0, 1), (NOT_FOUND, 0, 0, 1)]
    out.append(("deleted anchor", [u.export()], pq, pw, [(0, TEXT, 1, LEFT)], [(OK, (8, 2), LEFT, 1)]))
    # astral characters: pos_utf16 != pos
    a = wire.Replica(9)
    a.text_insert("text", 0, "a\U0001F600b\U0001F601中c"); a.commit()
    a.text_delete("text", 2, 1); a.commit()          # "a😀😁中c"; b (9,2) is a tombstone behind one astral scalar
    pq = [(0, TEXT, (9, c), LEFT) for c in range(6)] + [(0, TEXT, None, RIGHT)]
    pw = [(OK, 0, 0, -1), (OK, 1, 1, -1), (DELETED, 2, 3, -1), (OK, 2, 3, -1), (OK, 3, 5, -1), (OK, 4, 6, -1), (OK, 5, 7, 1)]
    out.append(("astral", [a.export()], pq, pw, [(0, TEXT, 3, MIDDLE), (0, TEXT, 5, MIDDLE)], [(OK, (9, 4), MIDDLE, 3), (OK, None, RIGHT, 5)]))
    # a child Text inside a Map, a Map, a MovableList, a wrong name, an empty container
    n = wire.Replica(11)
    child = n.map_set_container("m", "k", wire.KIND_TEXT)      # op (11, 0)
    n.text_insert(child, 0, "hey"); n.text_delete(child, 1, 1); n.mlist_insert("ml", 0, [1, 2]); n.commit()   # h1 e2 y3, delete = op 4
    n.text_insert("gone", 0, "zz"); z0 = n.seq[wire.root_cid("gone", wire.KIND_TEXT)][0]; n.text_delete("gone", 0, 2); n.commit()
    ckey = "cid:%d@%d:Text" % (child.counter, child.peer)
    pq = [(0, ckey, (11, 1), MIDDLE), (0, ckey, (11, 3), MIDDLE), (0, ckey, (11, 2), MIDDLE), (0, ckey, (11, 0), MIDDLE), (0, ckey, None, RIGHT),
          (0, "cid:root-m:Map", (11, 0), MIDDLE), (0, "cid:root-ml:MovableList", (11, 5), MIDDLE), (0, "cid:root-nope:Text", (11, 1), MIDDLE),
          (0, "cid:1@11:Text", (11, 1), MIDDLE), (0, "root-text", (11, 1), MIDDLE), (0, "cid:root-gone:Text", None, MIDDLE), (0, "cid:root-gone:Text", z0, RIGHT)]
    pw = [(OK, 0, 0, 0), (OK, 1, 1, 0), (DELETED, 1, 1, -1), (NOT_FOUND, 0, 0, 0), (OK, 2, 2, 1),
          (UNSUPPORTED, 0, 0, 0), (UNSUPPORTED, 0, 0, 0), (NO_CONTAINER, 0, 0, 0),
          (NO_CONTAINER, 0, 0, 0), (NO_CONTAINER, 0, 0, 0), (OK, 0, 0, 0), (DELETED, 0, 0, -1)]
    aq = [(0, ckey, 1, LEFT), (0, "cid:root-gone:Text", 0, MIDDLE), (0, "cid:root-gone:Text", 4, RIGHT), (0, "cid:root-m:Map", 0, LEFT), (0, "cid:root-nope:List", 0, LEFT)]
    aw = [(OK, (11, 3), LEFT, 1), (OK, None, LEFT, 0), (OK, None, RIGHT, 0), (UNSUPPORTED, None, LEFT, 0), (NO_CONTAINER, None, LEFT, 0)]
    out.append(("containers", [n.export()], pq, pw, aq, aw))
    return out


def chain_case(n_ops=3000, seed=3):
    """ONE writer, one chain, long enough for the batch kernels' linear prefix (which drops what it deletes from the leaves)"""
    rng = random.Random(seed)
    r = wire.Replica(21)
    for _ in range(n_ops):
        ids = r.seq.setdefault(wire.root_cid("text", wire.KIND_TEXT), [])
        if ids and rng.random() < 0.3:
            pos = rng.randrange(len(ids))
            r.text_delete("text", pos, min(len(ids) - pos, rng.randint(1, 3)))
        else:
            r.text_insert("text", rng.randint(0, len(ids)), rng.choice(["a", "bc", "\U0001F600", "déf"]))
        if rng.random() < 0.2:
            r.commit()
    r.commit()
    return [r.export()]


def sample_queries(doc, cid, ex, rng, n):
    """n ids of the container (visible ones and tombstones alike) + the fixed extras, with their answers"""
    ids = rng.sample(ex.order, min(n, len(ex.order)))
    tomb = [i for i in ex.order if i not in ex.vis]
    ids += rng.sample(tomb, min(max(4, n // 4), len(tomb)))
    pq = [(doc, cid, i, rng.choice((LEFT, MIDDLE, RIGHT))) for i in ids] + [(doc, cid, None, RIGHT), (doc, cid, (1, 0), LEFT)]
    aq = [(doc, cid, rng.randrange(ex.length + 2), rng.choice((LEFT, MIDDLE, RIGHT))) for _ in range(max(4, n // 4))]
    return pq, [ex.pos_answer(q[2], q[3]) for q in pq], aq, [ex.at_answer(q[2], q[3]) for q in aq]


def resident_pair(seed, n=120):
    """a writer's history, then a second step: the writer goes on while another peer edits concurrently in front of and inside what
    the first step left.  Returns (first step's blobs, second step's blobs)"""
    rng = random.Random(seed)
    a, b = wire.Replica(1000 + 2 * seed), wire.Replica(1001 + 2 * seed)

    def edit(r, k):
        for _ in range(k):
            ids = r.seq.setdefault(wire.root_cid("text", wire.KIND_TEXT), [])
            if ids and rng.random() < 0.3:
                pos = rng.randrange(len(ids))
                r.text_delete("text", pos, min(len(ids) - pos, rng.randint(1, 3)))
            else:
                r.text_insert("text", rng.randint(0, len(ids)), rng.choice(["ab", "c", "\U0001F600", "xyz "]))
            if rng.random() < 0.3:
                r.commit()
        r.commit()
    edit(a, n)
    first = a.export()
    vv1 = dict(a.vv)
    b.merge_from(a); b.set_visible("text", wire.KIND_TEXT, _oracle.visible_ids([first], "text", wire.KIND_TEXT))
    edit(b, n // 2)
    edit(a, n // 2)
    own_b = wire.Replica(b.peer); own_b.changes = {b.peer: b.changes[b.peer]}
    return [first], [a.export(from_vv=vv1), own_b.export()]
