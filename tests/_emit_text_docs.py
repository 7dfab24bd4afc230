"""Documents for the span-granular Text renderer (lm_k_emit.h, emit_doc, `kind == CK_TEXT && d.span`): shared by the kernel-logic test
(tests/test_emu_emit_text.py) and the GPU test (tests/test_gpu_zz_emit_text.py).

The renderer flattens the visible runs of a leaf 256 elements per step, four consecutive elements per lane: one run search per lane,
one 32-bit load when the four lie in one run, the short escapes expanded in registers, the step's bytes placed in an LDS window and
stored as aligned 16-byte pieces.  A step that holds a byte it does not expand (a scalar beyond ASCII, a style anchor, a control
character written \\u00XX) is rendered one element per lane.  The documents put run boundaries, escapes, those bytes and the output
position at every offset of that scheme.  Every document has ONE writer (a linear history), so the writer's own view is the
document and no file holds a decision of the oracle or of a kernel; the expected bytes are the oracle's and the plain model's."""
import functools

import _fuzz, _merge_ref, _richtext_ref
from loro_amd import wire

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1100)
SHORT_ESCAPES = '"\\\n\t\r\b\f'
STEP = 256     # elements of a step
LANE = 4       # elements of a lane


def _letters(n, off=0):
    return "".join(chr(ord("a") + (off + i) % 26) for i in range(n))


def _cut(s, lens):
    """s in chunks whose lengths cycle through `lens`"""
    out, i, k = [], 0, 0
    while i < len(s):
        out.append(s[i:i + lens[k % len(lens)]])
        i += lens[k % len(lens)]
        k += 1
    return out


def write_runs(r, target, chunks, deleted=(), commit_every=16):
    """Text `target` of replica `r` := the chunks in order, each chunk an item of its own: they are inserted back to front, every one
    at position 0, so no two have consecutive ids in sequence order and none merges with its neighbour.  The chunks whose index is in
    `deleted` are then deleted whole, right to left: runs of visible length 0 that stay in the leaf."""
    for i, c in enumerate(reversed(chunks)):
        if c:
            r.text_insert(target, 0, c)
        if i % commit_every == commit_every - 1:
            r.commit()
    starts, at = [], 0
    for c in chunks:
        starts.append(at)
        at += len(c)
    for i in sorted(set(deleted), reverse=True):
        if chunks[i]:
            r.text_delete(target, starts[i], len(chunks[i]))
    r.commit()


def runs_doc(chunks, deleted=(), name="text", peer=7):
    r = wire.Replica(peer)
    write_runs(r, name, chunks, deleted)
    return _fuzz.blobs_of([r]), [r]


def text_doc(s, lens=None, name="text", peer=7):
    return runs_doc(_cut(s, lens) if lens else [s], name=name, peer=peer)


def marked_doc(n, marks, peer=9):
    """a text of n letters in runs of 1-5, then marks: each adds a start and an end anchor, which take a position each"""
    r = wire.Replica(peer)
    write_runs(r, "text", _cut(_letters(n), (3, 1, 5, 2, 4)))
    for i, (a, b) in enumerate(marks):
        r.text_mark("text", a, b, "bold" if i % 2 == 0 else "link", True if i % 2 == 0 else "u%d" % i)
    r.commit()
    return _fuzz.blobs_of([r]), [r]


def model_result(reps, frontiers=None):
    return _merge_ref.Model(_richtext_ref.changes_of(reps)).result(frontiers)


# ---- 1. lengths
def _lengths():
    out = []
    for n in LENGTHS:
        s = _letters(n)
        if n == 0:
            out.append(runs_doc(["gone"], deleted=[0]))     # the root exists and shows nothing
            continue
        out.append(text_doc(s))                             # one run
        out.append(text_doc(s, (1, 2)))                     # runs of one and two: 1,100 elements are 734 items, several leaves
    return out


# ---- 2. run lengths against the lane groups
MIXED = (1, 3, 2, 5, 4, 7, 1, 1, 2, 6, 3, 9)


def _with_breaks(n):
    return "".join("\n" if i % 37 == 36 else c for i, c in enumerate(_letters(n)))


def _runs():
    out = []
    for lens in ((1,), (2,), (3,), (4,), (5,), MIXED):
        chunks = _cut(_with_breaks(330), lens)
        k = len(chunks)
        out.append(runs_doc(chunks))
        out.append(runs_doc(chunks, deleted=[i for i in range(k) if i % 3 == 1]))
        out.append(runs_doc(chunks, deleted=[i for i in range(k) if i % 7 in (2, 3)]))               # two in a row
        out.append(runs_doc(chunks, deleted=[i for i in range(k) if i % 11 in (4, 5, 6)]))           # three in a row
        out.append(runs_doc(chunks, deleted=[0, k - 1] + [i for i in range(k) if i % 64 in (0, 63)]))  # first and last of the text and of 64-item groups
        out.append(runs_doc(chunks, deleted=[i for i in range(k) if i % 5 != 2]))                    # mostly gone
        short = _cut(_with_breaks(400), lens)[:60]                                                   # one leaf
        out.append(runs_doc(short))
        out.append(runs_doc(short, deleted=[0, 59] + [i for i in range(60) if i % 9 in (3, 4, 5) or i % 13 == 7]))
    out.append(runs_doc(_cut(_letters(40), (3,)), deleted=range(14)))                               # everything deleted, run by run
    return out


# ---- 3. escapes
def _escapes():
    out = []
    for c in SHORT_ESCAPES + "\x7f":
        for pos in (0, 1, 2, 3, 255, 256, 257):
            s = _letters(300)
            out.append(text_doc(s[:pos] + c + s[pos:]))
        out.append(text_doc("".join(c if i % 5 == 0 else x for i, x in enumerate(_letters(70))), (1, 2, 3)))
    for m in range(4):
        out.append(text_doc(_letters(m) + '\n"\\\t' + _letters(9)))                   # eight bytes from one lane
        out.append(text_doc(_letters(m) + "\n" * 256 + _letters(5)))                  # 512 bytes from one step
        out.append(text_doc(_letters(m) + '"\\' * 200 + _letters(5), (1, 4, 2)))
    out.append(text_doc("\n" * 256))
    out.append(text_doc('"' * 1024))
    for c in "\x01\x1f\x00\x0b":                                                      # \u00XX: the step is rendered per element
        for m in range(4):
            out.append(text_doc(_with_breaks(256 + m) + c + _with_breaks(300)))
            out.append(text_doc(_letters(m) + c + '\n"' + _letters(3), (2, 1)))
    return out


# ---- 4. beyond ASCII
WIDE = ("é", "中", "😀")


def _wide():
    out = []
    for w in WIDE:
        out.append(text_doc(_with_breaks(300) + w + _with_breaks(300)))               # alone in its step
        for m in range(4):
            out.append(text_doc(_letters(m) + "\n" + w + '"\\' + w + "\t" + _letters(7), (2, 3, 1)))
    out.append(text_doc("".join(WIDE) * 90, (4, 1, 3)))
    for m in range(4):                                                                 # anchors at each position modulo 4
        out.append(marked_doc(600, [(m, 40 + m), (256 + m, 300), (8 + m, 12 + m), (520 + 2 * m, 560 + 3 * m)]))
        out.append(marked_doc(12 + m, [(m, 6 + m)]))
    return out


# ---- 5. output alignment
def _alignment():
    out = []
    body = _with_breaks(290) + '"q\\'
    for k in range(1, 18):                                                             # the first text byte at every offset modulo 16
        out.append(text_doc(body, (5, 2, 4), name="r" * k))
        out.append(text_doc(body[:k + 3], name="n" * k))
    r = wire.Replica(11)
    for i, nm in enumerate(("a", "bb", "ccccc")):
        write_runs(r, nm, _cut(_with_breaks(261 + 7 * i), (i + 2, 1)), deleted=[i + 1])
    out.append((_fuzz.blobs_of([r]), [r]))
    r = wire.Replica(12)                                                               # a Text as a Map value and as a List item
    t1 = r.map_set_container("m", "body", wire.KIND_TEXT)
    write_runs(r, t1, _cut(_with_breaks(300) + '"', (3, 2)), deleted=[2, 3])
    r.map_set("m", "n", 5)
    r.list_insert("l", 0, [1, "two"])
    t2 = r.list_insert_container("l", 1, wire.KIND_TEXT)
    write_runs(r, t2, _cut(_letters(270) + "\n\\é" + _letters(260), (4, 4, 1)))
    t3 = r.list_insert_container("l", 0, wire.KIND_TEXT)
    write_runs(r, t3, ["x"])
    r.commit()
    out.append((_fuzz.blobs_of([r]), [r]))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> list of (blobs, replicas), built once per process"""
    out = {"lengths": _lengths(), "runs": _runs(), "escapes": _escapes(), "wide": _wide(), "alignment": _alignment()}
    _check_corpus(out)
    return out


def all_docs():
    return [d for g in corpus().values() for d, _ in g]


def slab_docs():
    """documents of different JSON lengths for LM_SLAB_CAP: short ones that fit a middling slab, long ones that do not"""
    c = corpus()
    return [c["lengths"][i][0] for i in (0, 1, 5, 12)] + [c["runs"][i][0] for i in (1, 8)] + [c["escapes"][i][0] for i in (0, 60)] + \
           [c["wide"][0][0], c["alignment"][-1][0]]


@functools.lru_cache(maxsize=None)
def slab_edge_doc():
    """a document whose JSON is one byte longer than a multiple of 16: slabs are whole 16-byte pieces, so a slab of one byte less is
    the largest that overflows"""
    for n in range(290, 306):
        doc, reps = text_doc(_with_breaks(n) + '"\\', (6, 3))
        if len(model_result(reps)[1]) % 16 == 1:
            return doc
    raise AssertionError("no length in the range gives the remainder")


def version_session():
    """one document delivered in two imports, rendered at the first import's version after the second and then at the latest: in the
    resident tracker the second import's items are future at the checkout and its deletes do not count there (the renderer's other
    mask, ST_FUT | ST_DELMASK).  Returns [(blobs, frontiers)]"""
    r = wire.Replica(21)
    steps, seen = [], {}

    def deliver():
        nonlocal seen
        r.commit()
        steps.append(([r.export(seen)], None))
        seen = dict(r.vv)
        return list(r.frontiers)

    chunks = _cut(_with_breaks(280) + '"\\', (3, 1, 4, 2))
    write_runs(r, "text", chunks, deleted=[4, 5, 9])
    v0 = deliver()
    for i in range(30):                                   # new items between the old ones, old runs deleted in part and whole
        r.text_insert("text", 7 * i + 1, "N\n"[: 1 + i % 2] + "Q")
    for i in range(12):
        r.text_delete("text", 300 - 21 * i, 1 + i % 5)
    v1 = deliver()
    steps.append(([], wire.encode_frontiers(v0)))
    steps.append(([], None))
    steps.append(([], wire.encode_frontiers(v1)))
    return steps


# ---- what the corpus must contain, counted over the plain model's items
def model_items(reps, cid):
    """[(visible length, text)] of the items of `cid` in sequence order: maximal stretches of elements with consecutive ids of one
    peer and the same visibility — the runs a span-granular leaf holds, as long as the document fits one leaf"""
    m = _merge_ref.Model(_richtext_ref.changes_of(reps))
    V = m.version(None)
    items, prev = [], None
    for e in m.seqs.get(cid, ()):
        vis = _merge_ref._visible(e, V)
        ch = e.what[1] if e.what[0] == "char" else None     # None: a style anchor
        if prev is not None and prev[0] == (e.id[0], e.id[1] - 1) and prev[1] == vis:
            items[-1][1].append(ch)
        else:
            items.append([vis, [ch]])
        prev = (e.id, vis)
    return [(len(chs) if vis else 0, chs if vis else []) for vis, chs in items]


def _plain(ch):
    """the four-wide step expands this element itself"""
    return ch is not None and (0x20 <= ord(ch) < 0x80 or ch in "\b\t\n\f\r")


def corpus_counts(groups):
    """over the root Texts of the documents whose items fit one leaf (at most 64): lanes whose four positions span two runs, three or
    four runs, steps that hold an element the four-wide path does not expand, steps with an escape that it does"""
    two = more = fallback = fast_esc = 0
    for g in groups.values():
        for _, reps in g:
            m = _merge_ref.Model(_richtext_ref.changes_of(reps))
            for cid in m.sequences():
                if cid.kind != wire.KIND_TEXT:
                    continue
                items = model_items(reps, cid)
                if len(items) > 64:
                    continue
                owner, flat = [], []
                for i, (n, chs) in enumerate(items):
                    owner += [i] * n
                    flat += chs
                for l0 in range(0, len(flat), LANE):
                    k = len(set(owner[l0:l0 + LANE]))
                    two += k == 2
                    more += k >= 3
                for s0 in range(0, len(flat), STEP):
                    step = flat[s0:s0 + STEP]
                    if not all(_plain(c) for c in step):
                        fallback += 1
                    elif any(c in SHORT_ESCAPES for c in step):
                        fast_esc += 1
    return two, more, fallback, fast_esc


def _check_corpus(groups):
    two, more, fallback, fast_esc = corpus_counts(groups)
    assert two >= 50, two
    assert more >= 20, more
    assert fallback >= 20, fallback
    assert fast_esc >= 20, fast_esc
