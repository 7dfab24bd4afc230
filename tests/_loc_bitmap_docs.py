"""Documents for the kept[] bitmap of the span-granular tracker's loc[] (lm_k_integrate_span.h sp_keep / ts_loc_find): shared by the
kernel-logic test (tests/test_emu_loc_bitmap.py) and the GPU test (tests/test_gpu_zz_loc_bitmap.py).  The writers' views come from the
plain merge model (_merge_ref.view), so no document holds a decision of the oracle or of a kernel.

loc[] keeps an entry for the head of every item and for every element whose counter is a multiple of 64; an element is found by id
through the nearest kept entry at or below it in its 64-counter window.  The documents put lookups, cuts and clears at the edges of
that scheme: window boundaries, runs with more than four multiples of 64, slices of neighbouring documents, a second replay of the
same slice, trackers kept between runs."""
import functools
import random

import _fuzz, _merge_ref, _richtext_ref
from loro_amd import wire

TEXT = wire.root_cid("text", wire.KIND_TEXT)
WINDOW_EDGES = [(0, 1), (0, 63), (1, 0), (1, 1), (5, 0), (5, 1), (6, 5)]     # A's run holds 64 k + r elements
EDGE_COUNTERS = (0, 62, 63, 64, 65, 319, 320, 321)                         # … and its last one
NEIGHBOUR_TOTALS = (1, 31, 32, 33, 127, 128, 129, 4095, 4097)
BALLAST = 80


def _refresh(r):
    r.set_visible("text", wire.KIND_TEXT, _merge_ref.view(r, TEXT))


def _sync(a, b):
    a.commit(); b.commit()
    if a.merge_from(b):
        _refresh(a)


def _letters(n, off=0):
    return "".join(chr(ord("a") + (off + i) % 26) for i in range(n))


def model_result(reps, frontiers=None):
    return _merge_ref.Model(_richtext_ref.changes_of(reps)).result(frontiers)


def window_edge_doc(k, r, pa=11, pb=7):
    """A types ONE run of 64 k + r elements.  B knows its first few elements when it starts a branch of its own (a sibling of the rest
    of A's run); later B knows all of it, inserts behind and deletes A's elements at the window edges, while A — which has seen
    nothing of B — inserts behind the same elements: siblings found by id, deletes by id, A's branch retreated and replayed."""
    n = 64 * k + r
    a, b = wire.Replica(pa), wire.Replica(pb)
    f = min(3, n)
    a.text_insert("text", 0, _letters(f)); a.commit()
    _sync(b, a)
    if n > f:
        a.text_insert("text", f, _letters(n - f, f)); a.commit()
    b.text_insert("text", f, "XY")
    if n > 1:
        b.text_delete("text", 0, 1)
    for i in range(BALLAST):        # single elements in front, an item each: the tracker gets more than one leaf, so that an
        b.text_insert("text", 0, "0123456789"[i % 10])   # element that is not in the cached leaf has to be found through loc[]
    b.commit()
    _sync(b, a)
    ctrs = sorted({c for c in EDGE_COUNTERS + (n - 1,) if c < n})
    for c in ctrs:
        a.text_insert("text", a.seq[TEXT].index((pa, c)) + 1, "q")
    a.commit()
    for c in ctrs:
        ids = b.seq[TEXT]
        if (pa, c) not in ids:      # (counter 0 when B's branch deleted it)
            continue
        i = ids.index((pa, c))
        b.text_insert("text", i + 1, "z")
        b.text_delete("text", i, 1)
        b.text_insert("text", 1, "w")   # (another leaf takes the cache between two edges)
    b.commit()
    return _fuzz.blobs_of([a, b]), [a, b]


def window_session(seed, n_base=300, n_steps=160, n_peers=3, windows=((64, 128), (192, 256)), targets=None):
    """a text of n_base elements typed as one run by the first peer; then concurrent edits that aim at two 64-counter windows of it — a
    window is looked up, an item in it is cut (a new head, a new bit), an element behind the cut is looked up again.  `targets`: the
    counters to aim at instead (the window edges of a run of n_base elements)"""
    rng = random.Random(seed)
    base = 1000 + seed * 10
    reps = [wire.Replica(base + i) for i in range(n_peers)]
    p0 = reps[0]
    done = 0
    while done < n_base:
        k = min(n_base - done, rng.randint(20, 50))
        p0.text_insert("text", done, _letters(k, done)); p0.commit()
        done += k
    for r in reps[1:]:
        _sync(r, p0)
    for _ in range(n_steps):
        r = rng.choice(reps)
        ids = r.seq.setdefault(TEXT, [])
        lo, hi = rng.choice(windows)
        target = (p0.peer, rng.choice(targets) if targets else rng.randrange(lo, hi))
        i = ids.index(target) if target in ids else (rng.randrange(len(ids)) if ids else 0)
        if ids and rng.random() < 0.45:
            r.text_delete("text", i, min(len(ids) - i, rng.randint(1, 2)))
        else:
            r.text_insert("text", min(i + 1, len(ids)), "".join(rng.choice(_fuzz.ALPHA) for _ in range(rng.randint(1, 3))))
        if rng.random() < 0.5:
            r.commit()
        if rng.random() < 0.2:
            x, y = rng.sample(reps, 2)
            _sync(x, y)
    for r in reps:
        r.commit()
    return _fuzz.blobs_of(reps), reps


def neighbour_doc(total, peer0):
    """a document whose ops hold `total` atoms: A types a run, then A and B insert single elements concurrently, in turn at the front
    and in the middle of the run (40 each where the total allows it: more than 64 items, so more than one leaf and lookups by id)"""
    a, b = wire.Replica(peer0 + 1), wire.Replica(peer0)
    if total < 3:
        a.text_insert("text", 0, _letters(total)); a.commit()
        return _fuzz.blobs_of([a]), [a]
    k = 40 if total >= 127 else 1
    n = total - 2 * k
    a.text_insert("text", 0, _letters(n)); a.commit()
    _sync(b, a)
    for r, ch in ((a, "Q"), (b, "z")):
        for i in range(k):
            r.text_insert("text", 0 if i % 2 else r.seq[TEXT].index((a.peer, n // 2)) + 1, ch)
        r.commit()
    return _fuzz.blobs_of([a, b]), [a, b]


def resident_session():
    """one document delivered in three imports with checkouts in between: the second import continues with the peers and the layout of
    the first (DF_LAYOUT_SAME: loc[] and kept[] are kept, only the new slots are cleared), the third brings a peer that sorts in front
    of the others (the stored leaves are renumbered, loc[] and kept[] are rebuilt).  Returns [(blobs, frontiers)]"""
    a, b, hub = wire.Replica(500), wire.Replica(400), wire.Replica(900)
    steps, versions, seen = [], [], {}

    def deliver(reps):
        nonlocal seen
        for r in reps:
            r.commit()
            hub.merge_from(r)
        steps.append(([hub.export(seen)], None))
        seen = dict(hub.vv)
        versions.append(list(hub.frontiers))

    a.text_insert("text", 0, _letters(150)); a.commit()
    _sync(b, a)
    b.text_insert("text", 70, "BB"); b.text_delete("text", 60, 3)
    a.text_insert("text", 66, "AA"); a.text_delete("text", 100, 2)
    deliver([a, b])
    steps.append(([], wire.encode_frontiers([(500, 149)])))
    steps.append(([], None))
    _sync(a, b); _sync(b, a)
    # old elements (A's windows 0 and 1) and new ones, concurrently
    ia = a.seq[TEXT].index((500, 64))
    a.text_insert("text", ia + 1, _letters(70, 3)); a.text_delete("text", ia - 2, 2)
    ib = b.seq[TEXT].index((500, 64))
    b.text_insert("text", ib + 1, "bbbb"); b.text_delete("text", ib + 8, 2); b.text_insert("text", 0, "h")
    deliver([a, b])
    steps.append(([], wire.encode_frontiers(versions[0])))
    steps.append(([], None))
    _sync(a, b); _sync(b, a)
    c = wire.Replica(300)           # sorts in front of both
    _sync(c, a)
    ic = c.seq[TEXT].index((500, 127))
    c.text_insert("text", ic + 1, "CCC"); c.text_delete("text", ic - 1, 2)
    na = a.next_counter
    a.text_insert("text", ia + 20, "xy"); a.text_delete("text", ic, 1)
    deliver([a, c])
    steps.append(([], wire.encode_frontiers(versions[1])))
    steps.append(([], None))
    assert na > 150
    return steps


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> list of (blobs, replicas), built once per process"""
    out = {
        "edges": [window_edge_doc(k, r) for k, r in WINDOW_EDGES],
        "edge_sessions": [window_session(100 + i, n_base=64 * k + r, n_steps=120, targets=[c for c in EDGE_COUNTERS + (64 * k + r - 1,) if c < 64 * k + r])
                          for i, (k, r) in enumerate(WINDOW_EDGES)],
        "windows": [window_session(seed) for seed in range(6)],
        "neighbours": [neighbour_doc(t, 2000 + 10 * i) for i, t in enumerate(NEIGHBOUR_TOTALS)],
        "retry": [window_session(40 + seed, n_steps=320) for seed in range(2)],
    }
    # the fuzz generator of the other suites, with a solo prefix: a linear prefix, then a tracker that builds loc[] at its first move
    out["fuzz"] = []
    for seed in (7001, 7002, 7003, 7004):
        reps = _fuzz.random_session(seed, n_peers=3, n_steps=120, kinds=("text",), solo_steps=100, max_ins=8, view=_merge_ref.view)
        out["fuzz"].append((_fuzz.blobs_of(reps), reps))
    return out


def mixed_batch():
    """plain text documents, a MovableList document, a checked-out document and a List with child containers: (docs, frontiers)"""
    c = corpus()
    docs = [d for d, _ in c["edges"][:3]] + [c["windows"][0][0]]
    fr = [None] * len(docs)
    docs.append(_fuzz.blobs_of(_fuzz.movable_session(40, n_steps=80, nested=True))); fr.append(None)
    snaps = []
    reps = _fuzz.random_session(61, n_peers=3, n_steps=100, kinds=("text", "list"), snapshots=snaps)
    assert snaps
    docs.append(_fuzz.blobs_of(reps)); fr.append(wire.encode_frontiers(snaps[len(snaps) // 2][0]))
    docs.append(_fuzz.blobs_of(_fuzz.nested_session(5, n_peers=3, n_steps=120))); fr.append(None)
    docs += [c["windows"][1][0], c["edges"][6][0]]; fr += [None, None]
    return docs, fr
