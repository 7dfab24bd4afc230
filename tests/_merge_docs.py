"""Documents for the tests of the plain merge model (tests/_merge_ref.py): fuzz corpora whose writers take their view from the
model (no decision of the oracle in them), hand-built documents aimed at the edges of the integrate kernels, and the checkout
versions of each.  Shared by tests/test_merge_ref.py (oracle, kernel-logic harness) and tests/test_gpu_zz_merge_ref.py."""
import random

import _fuzz, _merge_ref
from _richtext_ref import changes_of
from loro_amd import wire

TEXT = wire.root_cid("text", wire.KIND_TEXT)
V = _merge_ref.view


class Doc:
    """one document: its blobs, the model of it and the versions it is checked out at"""

    def __init__(self, label, reps, snaps=(), n_versions=4):
        self.label = label
        self.snaps = [(list(fr), blob) for fr, blob in snaps]          # (frontiers, updates holding exactly that version or None)
        self.blobs = _fuzz.blobs_of(reps)
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
    tot = dict.fromkeys(_merge_ref.OUTCOMES, 0)
    for d in docs:
        for k, v in d.model.stats.items():
            tot[k] += v
    return tot


def check_conditions(name, docs):
    """asserted from the model alone, before anything is compared: a corpus cannot pass by being boring"""
    tot = outcome_counts(docs)
    for k in _merge_ref.OUTCOMES:
        assert tot[k] >= (1 if k == "diff_right_equal" else 50), (name, k, tot)
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
