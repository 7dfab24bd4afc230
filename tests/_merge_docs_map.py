"""LWW Map documents for the tests of the plain merge model against k_map_fused (lm_k_map_fused.h), the kernel that decodes Map
blocks WITHOUT op rows.  Every document is written with wire.Replica or raw wire.Change / wire.encode_updates([[...]]); its model
comes from the writers' changes (`changes_of(reps)`); no decision of the oracle is in any of them.  Shared by
tests/test_merge_ref_map.py (oracle, kernel-logic harness) and tests/test_gpu_zz_merge_ref_map.py.

Every hand-built GROUP knows its path: STAYS = k_map_fused decides every document (fused == len, redo == 0), LEAVES = every document
is handed to the side engine (DF_REDO: fused == len, redo == len), ROWS = k_doc_kind does not take the documents at all (fused == 0).
Where the source names a limit the side comes from that constant (LIMITS below, checked against the source text by
test_merge_ref_map.py::test_limits_are_the_sources); where it names none the path was observed once on the kernel-logic harness and
is asserted since, harness and GPU alike:
  * integers of ten sleb128 bytes (2^62 … i64 max / min): STAY — mf_values_int_all refuses them, mf_chain<false> reads them;
  * keys of 32, 33, 127, 128 and 300 bytes, keys with a tab / 0x7f, non-ASCII keys: STAY — the candidate test fails, mf_chain<true> reads them;
  * child Map containers (tag 9), also two concurrent ones under one key, also 31 of them in one block: STAY;
  * a nested list / map value (tags 7 / 8): LEAVES;
  * a key table with more bytes below 0x20 than MF_KMAX (300 keys of four tabs each): LEAVES although it holds 301 entries — the
    key-start scan counts its candidates against MF_KMAX before it verifies them (the source says so since); with spaces: STAYS;
  * documents with pending changes (a missing peer, a blob missing from the middle): STAY;
  * one peer more than k_doc_tables takes (MAX_PEERS - 1 = 255): "refused" — LM_UNSUPPORTED and no rendering; the document counts as
    fused and as handed over (the side engine's decoders own every error code), fused == redo == len.

Fuzz corpora (map_corpora): the fewest seeds, in steps of ten, at which check_map_conditions holds — counted by the model at the
latest version (checkout differs: over the first two versions of each document, the ones the harness and the device receive),
per corpus (70 / 30 / 50 seeds):
  "2 peers"   concurrent keys 238, lamport ties 26, won by the last delivered 10, by the first 16, delete wins 603, child maps hidden 22, checkout differs 427
  "4 peers"   concurrent keys 251, lamport ties 22, won by the last delivered 12, by the first 10, delete wins 242, child maps hidden 23, checkout differs 173
  "1-6 peers" concurrent keys 294, lamport ties 32, won by the last delivered 20, by the first 12, delete wins 425, child maps hidden 34, checkout differs 330
What binds is a tie won by the peer whose blob comes last (first): "2 peers" has 8 at 60 seeds, "4 peers" 9 (won by the first) at 20,
"1-6 peers" 9 (won by the first) at 40.  A tie needs two writes to one key at the same lamport that have not seen each other; a write
that has seen the other side has a greater lamport, so ties only arise between peers that start from the same version."""
import os, random, re

import _fuzz, _merge_ref
from _richtext_ref import changes_of
from loro_amd import wire

K = wire
STAYS, LEAVES, ROWS = "stays", "leaves", "rows"
FORCE = {"LM_MF_MIN_ROWS": "1", "LM_MF_CHG_RATIO": "0"}      # the product thresholds (2,048 rows, 4 rows per change) keep small documents out


def _source(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "loro_amd", "csrc", name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


def limits():
    """the limits k_map_fused and its host state, read from the source text (so that a changed constant moves the documents with it)"""
    mf, ty, lw, dec = _source("lm_k_map_fused.h"), _source("lm_types.h"), _source("lm_k_lww_doc.h"), _source("lm_k_decode.h")
    out = {"MF_KMAX": _const(mf, "MF_KMAX"), "MF_RMAX": _const(mf, "MF_RMAX"), "MAX_PEERS": _const(ty, "MAX_PEERS"), "LWW_LDS_CAP": _const(lw, "LWW_LDS_CAP")}
    assert "if (klen_sec > 0xfff0u) bail = true;" in mf and "if (send - sec > 0xfff0u) return NONE;" in mf
    out["SECTION"] = 0xfff0
    assert "if (ncid == 0 || ncid > 32) ok = false;" in dec
    out["CONTAINERS"] = 32
    assert "if (at >= cap / 2) s_misc[1] = 1;" in mf            # the (cap / 2 + 1)-th distinct pair gives the table up
    assert "if (P >= MAX_PEERS - 1) { too_many = true; break; }" in _source("lm_k_dag.h")    # k_doc_tables: MAX_PEERS - 1 peers at most
    return out


LIMITS = limits()


def table_cap(n_rows, ht_opt=None):
    """the host's choice of a document's LDS table (lm_pipeline.h: 64 doubled until it holds 2 x the Map rows, capped by LM_HT_OPT)"""
    cap = 64
    while cap < 2 * n_rows:
        cap <<= 1
    return min(cap, ht_opt if ht_opt is not None else LIMITS["LWW_LDS_CAP"])


class MapDoc:
    """one document: blobs, the model of it, the versions it is checked out at, the peers in the order of their blobs"""

    def __init__(self, label, reps, blobs=None, versions=(), delivered=None, changes=None):
        self.label, self.reps = label, reps
        self.blobs = _fuzz.blobs_of(reps) if blobs is None else blobs
        self.model = _merge_ref.Model(changes_of(reps) if changes is None else changes, delivered=delivered)
        self.versions = [list(v) for v in versions]
        self.delivery = [r.peer for r in reps if r.changes.get(r.peer)]

    def whole_exports(self):
        """the same document as every replica's WHOLE export: the histories overlap, known changes are dropped on import"""
        o = MapDoc.__new__(MapDoc)
        o.__dict__.update(self.__dict__)
        o.label, o.blobs = self.label + ", whole exports", [r.export() for r in self.reps if r.changes]
        return o


def block_blob(r):
    """every change of `r`'s own in ONE block (Replica.export cuts blocks at about 512 Map rows)"""
    return wire.encode_updates([r.changes[r.peer]])


def ends_of(reps, every=1):
    return [[(r.peer, c.ctr_end - 1)] for r in reps for c in r.changes.get(r.peer, [])[::every]]


def sync(*reps):
    for r in reps:
        r.commit()
    for a in reps:
        for b in reps:
            if a is not b:
                a.merge_from(b)


# ------------------------------------------------------------------------------------------------------------------- fuzz corpora
def scalar(rng):
    kind = rng.randrange(9)
    if kind == 0:
        return rng.choice([None, True, False])
    if kind == 1:
        return rng.choice([-1, 1]) * (1 << rng.randrange(0, 63)) + rng.randint(-2, 2)
    if kind == 2:
        return rng.randint(-70, 70)
    if kind == 3:
        return rng.random() * 10 ** rng.randint(-5, 9)
    if kind == 4:
        return "x" * rng.choice([0, 1, 62, 63, 64, 65, 200])
    if kind == 5:
        return rng.choice(["s%d" % rng.randint(0, 999), "\x03\x03\x03", "é中😀", "q\"\\\n"])
    if kind == 6:
        return bytes(rng.randrange(256) for _ in range(rng.randint(0, 5)))
    if kind == 7:
        return 3
    return float(rng.randint(-5, 5))


def map_session(seed, n_peers, n_steps=120, sync_prob=0.08, all_sync_prob=0.06):
    """Random concurrent session over one to three root Maps and child Maps made by map_set_container (written into by every peer
    that has seen their creating op): sets of every scalar kind, deletes, pairwise syncs.  Few keys, so that most are contested;
    every peer starts at lamport 0, so ties are common.  -> (reps, versions)"""
    rng = random.Random(seed)
    reps = [wire.Replica(p) for p in rng.sample([1, 2, 3, 5, 70, 90, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, rng.randrange(1 << 64)], n_peers)]
    conts = [(wire.root_cid("m%d" % i, K.KIND_MAP), None) for i in range(rng.randint(1, 3))]
    keys = ["k%d" % i for i in range(rng.randint(2, 6))] + rng.sample(["", "ключ", "abcdefgh", "abcdefg", "abcdefgX", "a b", "0123456789abcdef0123456789abcde"], 2)
    versions = []

    def usable(r):
        return [c for c, made in conts if made is None or r.vv.get(made[0], 0) > made[1] or made[0] == r.peer]
    for step in range(n_steps):
        r = rng.choice(reps)
        cid = rng.choice(usable(r))
        key = rng.choice(keys)
        x = rng.random()
        if x < 0.18:
            r.map_delete(cid, key)
        elif x < 0.28 and len(conts) < 14:
            child = r.map_set_container(cid, key, K.KIND_MAP)
            conts.append((child, (child.peer, child.counter)))
            r.map_set(child, rng.choice(keys), scalar(rng))
        else:
            r.map_set(cid, key, scalar(rng))
        if rng.random() < 0.3:
            r.commit()
            if rng.random() < 0.3:
                versions.append(list(r.frontiers))
            elif rng.random() < 0.3:
                ch = r.changes[r.peer][-1]
                versions.append([(r.peer, rng.randrange(ch.counter, ch.ctr_end))])        # (in the middle of a change)
        if n_peers > 1 and rng.random() < sync_prob:
            a, b = rng.sample(reps, 2)
            a.commit(); b.commit(); a.merge_from(b)
        if n_peers > 1 and rng.random() < all_sync_prob:       # everyone meets: the next writes of all peers share their lamports
            sync(*reps)
    for r in reps:
        r.commit()
    own = [r for r in reps if r.changes.get(r.peer)]
    if len(own) > 1:                                                                     # (a two-peer frontier)
        a, b = rng.sample(own, 2)
        versions.append(sorted([(a.peer, rng.randrange(a.vv[a.peer])), (b.peer, rng.randrange(b.vv[b.peer]))]))
    return reps, versions


def map_corpora():
    out = {}
    for name, seeds, peers in (("2 peers", range(1000, 1070), lambda s: 2), ("4 peers", range(2000, 2030), lambda s: 4), ("1-6 peers", range(3000, 3050), lambda s: 1 + s % 6)):
        out[name] = []
        for s in seeds:
            reps, versions = map_session(s, peers(s))
            out[name].append(MapDoc("%s seed %d" % (name, s), reps, versions=versions))
    return out


MAP_AT_LEAST = {"concurrent_keys": 50, "tie_on_lamport": 20, "tie_won_by_last_delivered": 10, "tie_won_by_first_delivered": 10, "winner_is_delete": 20,
                "child_map_hidden": 10, "checkout_winner_differs": 10}


RUN_VERSIONS = 2      # versions of a corpus document that the harness and the device are given (the oracle comparison takes all)


def map_outcome_counts(docs):
    """checkout_winner_differs is counted over the versions the kernels receive, `versions[:RUN_VERSIONS]`"""
    tot = dict.fromkeys(_merge_ref.MAP_OUTCOMES, 0)
    for d in docs:
        for k, v in d.model.map_outcomes(d.delivery, d.versions[:RUN_VERSIONS]).items():
            tot[k] += v
    return tot


def check_map_conditions(name, docs):
    """asserted from the model alone, before anything is compared: a corpus cannot pass by being boring"""
    tot = map_outcome_counts(docs)
    for k, least in MAP_AT_LEAST.items():
        assert tot[k] >= least, (name, k, tot)
    return tot


# ----------------------------------------------------------------------------------------------------------- hand-built documents
def contested(label, keys, values=None, peers=(7, 5), one_block=True, versions=True, extra=None, max_rows=None):
    """Two (or more) peers write EVERY key of `keys` concurrently from lamport 0 — the first in the order given, the others rotated,
    so the lamports of a key's writes differ for most keys and tie for some — then the first peer deletes every seventh key having
    seen nothing of the others (with `max_rows`: as many of them as leave its block at that many rows).  One block per peer."""
    reps = [wire.Replica(p) for p in peers]
    values = values or [None]
    for j, r in enumerate(reps):
        n = len(keys)
        order = keys if j == 0 else [keys[(i + j * (n // 3 + 1)) % n] for i in range(n)] if j % 2 else keys[::-1]
        for i, k in enumerate(order):
            v = values[(i + j) % len(values)]
            r.map_set("m", k, ("%d:%d" % (j, i)) if v is None else v)
        r.commit()
    for k in keys[::7][:None if max_rows is None else max_rows - len(keys)]:
        reps[0].map_delete("m", k)
    reps[0].commit()
    if extra:
        extra(reps)
    blobs = [block_blob(r) for r in reps] if one_block else None
    return MapDoc(label, reps, blobs=blobs, versions=ends_of(reps) + [[(reps[1].peer, len(keys) // 2)], [(reps[0].peer, len(keys) // 3), (reps[1].peer, 0)]] if versions else ())


def n_table_keys(r):
    """entries of the key table of `r`'s one block: the root containers' names and the distinct keys"""
    seen = set()
    for c in r.changes[r.peer]:
        for o in c.ops:
            seen.add(o.key)
            if o.cid.root:
                seen.add(o.cid.name)
    return len(seen)


def key_section_len(r):
    seen = []
    for c in r.changes[r.peer]:
        for o in c.ops:
            for k in ([o.cid.name] if o.cid.root else []) + [o.key]:
                if k not in seen:
                    seen.append(k)
    return sum(len(wire.lbytes(k.encode("utf-8"))) for k in seen)


def keys_filling(total, key_len=300):
    """distinct keys whose section, together with the root name "m" (2 bytes), is exactly `total` bytes"""
    out, left = [], total - 2
    per = key_len + (1 if key_len < 128 else 2)
    while left >= 3 * per:
        out.append(("%05d" % len(out)).ljust(key_len, "k")); left -= per
    a = left // 2
    for n in (a, left - a):
        body = n - (1 if n - 1 < 128 else 2)
        assert n != 129 and body >= 5, n
        out.append(("%05d" % len(out)).ljust(body, "z"))
    return out


def key_docs():
    """-> [(group label, path, [MapDoc])]"""
    L = LIMITS
    stays = []
    lens = [0, 1, 7, 8, 9, 30, 31]
    stays.append(contested("key lengths 0-31 (candidate test)", ["".ljust(n, "abcdefghij"[n % 10]) for n in lens] + ["p%d" % i for i in range(9)]))
    stays.append(contested("key lengths 32-300 (chain)", ["%02d" % n + "".ljust(n - 2, "y") for n in (32, 33, 127, 128, 300)] + ["", "q", "short"]))
    stays.append(contested("all key lengths", ["%d|" % n + "".ljust(max(0, n - len("%d|" % n)), "w") for n in (1, 7, 8, 9, 30, 31, 32, 33, 127, 128, 300)] + [""]))
    stays.append(contested("equal length, equal first eight bytes", ["abcdefgh" + t for t in ("1", "2", "3")] + ["abcdefghij" * 3 + t for t in "xyz"] + ["12345678", "1234567"]))
    stays.append(contested("keys that differ in length only", ["abcdefg", "abcdefgh", "abcdefghi", "a", "ab", "", "abcdefg\x00"[:7] + "h" * 2]))
    stays.append(contested("tab, spaces, 0x7f, non-ASCII", ["tab\tkey", " ", "   ", "del\x7fkey", "\x7f", "ключ", "键", "😀😀", "e\u0301", "nul\x00key"]))
    for total in (255, 256, 257):
        stays.append(contested("key section of %d bytes" % total, keys_filling(total, 29)))
        assert key_section_len(stays[-1].reps[0]) == total
    for at in (255, 256):      # "m" (2 bytes), then 11-byte keys up to the offset, so that a length byte sits exactly at `at`
        n_full, rest = divmod(at - 2, 11)
        keys = ["%03d" % i + "abcdefg" for i in range(n_full - 1)] + ["L".ljust(10 + rest, "l")] + ["after%d" % i for i in range(6)]
        d = contested("a length byte at offset %d" % at, keys)
        sec = b"".join(wire.lbytes(k.encode()) for k in ["m"] + keys)
        assert sec[at] == 6 and sec[at + 1:at + 7] == b"after0", (at, sec[at])
        stays.append(d)
    # more bytes below 0x21 than MF_KMAX in a table of 300 keys: spaces are no candidates for a key start, the block stays …
    stays.append(contested("300 keys of four spaces each", ["a b c d %03d" % i for i in range(300)], versions=False))
    groups = [("keys", STAYS, stays)]
    # … tabs are: the candidate count passes MF_KMAX although the table holds 300 keys, and the block is handed over (lm_k_map_fused.h
    # "key starts": the candidates are counted before they are verified)
    groups.append(("more control characters than MF_KMAX", LEAVES, [contested("300 keys of four tabs each", ["a\tb\tc\td\t%03d" % i for i in range(300)], versions=False)]))
    for n in (L["MF_KMAX"] - 1, L["MF_KMAX"], L["MF_KMAX"] + 1):
        d = contested("%d entries in one key table" % n, ["k%d" % i for i in range(n - 1)], versions=False, max_rows=L["MF_RMAX"])
        assert n_table_keys(d.reps[0]) == n and sum(len(c.ops) for c in d.reps[0].changes[7]) == L["MF_RMAX"]
        groups.append(("%d key table entries" % n, STAYS if n <= L["MF_KMAX"] else LEAVES, [d]))
    for total in (L["SECTION"], L["SECTION"] + 1):
        d = contested("key section of %#x bytes" % total, keys_filling(total), versions=False)
        assert key_section_len(d.reps[0]) == total == key_section_len(d.reps[1])
        groups.append(("key section %#x" % total, STAYS if total <= L["SECTION"] else LEAVES, [d]))
    return groups


def column_docs():
    """the key-index column (DeltaRle) of one block"""
    docs = []
    rng = random.Random(5)
    for label, idx in (("one key repeated (a run of delta 0)", [1] * 300), ("ascending (a run of +1)", list(range(1, 400))),
                       ("random order (literals)", [rng.randrange(1, 60) for _ in range(700)]),
                       ("two-byte deltas of both signs", list(range(0, 1020)) + [0, 1019, 0, 1019]),
                       ("runs and literals mixed", [i // 5 if i % 40 < 20 else (i * 7) % 50 for i in range(900)])):
        a, b = wire.Replica(11), wire.Replica(4)
        for i, k in enumerate(idx):
            a.map_set("m", "m" if k == 0 else "k%d" % k, i)
        a.commit()
        for k in sorted(set(idx))[::3]:
            b.map_set("m", "m" if k == 0 else "k%d" % k, "b")
            if k % 2:
                b.map_delete("m", "m" if k == 0 else "k%d" % k)
        b.commit()
        docs.append(MapDoc(label, [a, b], blobs=[block_blob(a), block_blob(b)], versions=[[(11, len(idx) // 2)], [(11, len(idx) - 2), (4, 1)]]))
    for n in range(250, 262):       # one literal segment of n one-byte deltas: head (2 bytes) + n — its last terminator is byte n + 1 of the column, on both sides of 255 / 256
        rng = random.Random(n)
        a = wire.Replica(11)
        last = 1
        for i in range(n + 1):
            k = rng.choice([x for x in range(1, 40) if abs(x - last) > 1 or i == 0]); last = k
            a.map_set("m", "k%d" % k, i)
        a.commit()
        docs.append(MapDoc("a literal segment of %d deltas" % n, [a], blobs=[block_blob(a)], versions=[[(11, n // 2)]]))
    return [("key-index column", STAYS, docs)]


def int_edges(max_bytes):
    out = [0, 3, -3]
    for k in range(1, max_bytes + 1):
        e = 1 << (7 * k - 1) if k < 10 else 1 << 62
        out += [e - 1, e, -e, -e - 1]
    if max_bytes >= 10:
        out += [(1 << 63) - 1, -(1 << 63), (1 << 62) + 12345, -(1 << 62) - 1]
    return out


def value_docs():
    stays = []
    stays.append(contested("integers of one to nine bytes", ["i%d" % i for i in range(40)], int_edges(9)))
    stays.append(contested("integers of one to ten bytes", ["i%d" % i for i in range(52)], int_edges(10)))
    for v in int_edges(10)[-8:]:
        stays.append(contested("every value %d" % v, ["i%d" % i for i in range(5)], [v], versions=False))
    stays.append(contested("every value 3 (the payload byte equals the tag)", ["i%d" % i for i in range(70)], [3]))

    def one_delete(reps):
        b = reps[1]
        for i in range(30):
            b.map_set("m", "i%d" % i, i * 1000)
        b.map_delete("m", "i7")
        for i in range(30, 60):
            b.map_set("m", "i%d" % i, -i)
        b.commit()
    stays.append(contested("an all-integer block with one delete in the middle", ["i%d" % i for i in range(60)], [5, 70, -9000], extra=one_delete, one_block=False))
    mixed = ["", "x" * 63, "y" * 64, "z" * 65, "w" * 200, "\x03\x03\x03\x03", 1.5, -0.0, 1e300, 5e-324, True, False, None, b"", b"\x00\xff\x03", 3, "é中😀"]
    stays.append(contested("mixed scalars", ["v%d" % i for i in range(len(mixed) * 2 + 1)], mixed))
    for n in (61, 62, 63):           # tag + length byte + n bytes = 63 / 64 / 65: the next value starts at byte 63 / 64 of the chain's window / first of the next
        stays.append(contested("a value that starts at byte %d of a chain window" % (n + 2), ["v%d" % i for i in range(12)], ["s" * n, 7, None, "t" * n, 2.5]))
    # child Maps
    for pc, ps in ((9, 6), (6, 9)):
        x, p, q = wire.Replica(7), wire.Replica(pc), wire.Replica(ps)
        x.map_set("m", "k", 0); x.commit()
        sync(x, p, q)
        child = p.map_set_container("m", "k", K.KIND_MAP)
        p.map_set(child, "in", 1); p.commit()
        q.map_set("m", "k", "plain"); q.commit()
        vs = [[(p.peer, 0)], [(p.peer, 1)], [(q.peer, 0)], [(p.peer, 1), (q.peer, 0)]]
        sync(x, p, q)
        q.map_set(child, "late", 2); q.commit()
        d = MapDoc("a child Map against a concurrent scalar, the child's peer is the %s" % ("greater" if pc > ps else "smaller"), [x, p, q], versions=vs)
        assert d.model.value() == {"m": {"k": {"in": 1, "late": 2} if pc > ps else "plain"}}
        stays.append(d)
    x, p, q = wire.Replica(7), wire.Replica(3), wire.Replica(1 << 40)
    x.map_set("m", "other", 0); x.commit()
    sync(x, p, q)
    cp = p.map_set_container("m", "k", K.KIND_MAP); p.map_set(cp, "from", "p"); p.commit()
    cq = q.map_set_container("m", "k", K.KIND_MAP); q.map_set(cq, "from", "q"); q.commit()
    sync(x, p, q)
    p.map_set(cq, "p wrote", 1); p.map_set(cp, "p wrote", 2); q.map_set(cp, "q wrote", 3); q.map_set(cq, "q wrote", 4); p.commit(); q.commit()
    d = MapDoc("two concurrent child Maps under one key", [x, p, q], versions=[[(3, 0)], [(3, 1)], [(1 << 40, 1)], [(3, 1), (1 << 40, 1)], [(3, 2)]])
    assert d.model.value() == {"m": {"k": {"from": "q", "p wrote": 1, "q wrote": 4}, "other": 0}}
    stays.append(d)
    leaves = [contested("a nested list value", ["v%d" % i for i in range(9)], [1, [1, 2, "z"], "s"]),
              contested("a nested map value", ["v%d" % i for i in range(9)], [1, {"a": 1, "b": [2]}, "s"])]
    return [("values", STAYS, stays), ("nested values", LEAVES, leaves)]


def row_docs():
    L = LIMITS
    groups = []
    for n in (L["MF_RMAX"] - 1, L["MF_RMAX"], L["MF_RMAX"] + 1):
        a, b = wire.Replica(21), wire.Replica(12)
        for i in range(n):
            a.map_set("m", "k%d" % (i % 300), i)
        a.commit()
        for i in range(0, 300, 2):
            b.map_set("m", "k%d" % i, "b%d" % i)
        b.commit()
        d = MapDoc("a block of %d rows" % n, [a, b], blobs=[block_blob(a), block_blob(b)], versions=[[(21, n // 2)], [(21, n - 1)], [(21, 700), (12, 3)]])
        groups.append(("%d rows in one block" % n, STAYS if n <= L["MF_RMAX"] else LEAVES, [d]))
    docs = []
    for n in (63, 64, 65, 129):
        a, b = wire.Replica(21), wire.Replica(12)
        for c in range(n):
            for j in range(1 + c % 3):
                a.map_set("m", "k%d" % ((c * 5 + j) % 37), c * 10 + j)
            a.commit()
        for i in range(37):
            b.map_set("m", "k%d" % i, "b"); b.commit()
        docs.append(MapDoc("%d changes in one block" % n, [a, b], blobs=[block_blob(a), block_blob(b)],
                           versions=[[(21, a.changes[21][k].ctr_end - 1)] for k in (0, 62, 63, 64, n - 1) if k < n] + [[(21, a.changes[21][63 if n > 63 else 5].counter), (12, 20)]]))
    a, b = wire.Replica(21), wire.Replica(12)
    for c in range(12):
        a.map_set("m", "k%d" % c, c); a.commit()
    for i in range(1000):
        a.map_set("m", "k%d" % (i % 100), i)
    a.commit()
    for c in range(12):
        a.map_set("m", "k%d" % (c * 3), -c); a.commit()
    for i in range(100):
        b.map_set("m", "k%d" % i, "b")
        if i % 10 == 0:
            b.commit()
    b.commit()
    docs.append(MapDoc("changes of one row beside one of 1,000 rows", [a, b], blobs=[block_blob(a), block_blob(b)], versions=ends_of([a], 5) + [[(21, 500)], [(21, 1011), (12, 50)]]))
    groups.append(("changes", STAYS, docs))
    for n in (L["CONTAINERS"], L["CONTAINERS"] + 1):
        a, b = wire.Replica(21), wire.Replica(12)
        kids = [a.map_set_container("m", "c%d" % i, K.KIND_MAP) for i in range(n - 1)]
        for i, c in enumerate(kids):
            a.map_set(c, "k", i)
        a.commit()
        b.map_set("m", "c3", "plain"); b.map_set("m", "c4", "plain"); b.commit()
        sync(a, b)
        for i, c in enumerate(kids):
            b.map_set(c, "k2", -i)
        b.commit()
        d = MapDoc("%d containers in one block" % n, [a, b], blobs=[block_blob(a), block_blob(b)], versions=[[(21, n - 2)], [(21, n + 5)], [(12, 1)]])
        groups.append(("%d containers in one block" % n, STAYS if n <= L["CONTAINERS"] else ROWS, [d]))
    return groups


def table_docs(ht_opt=None):
    """distinct (container, key) pairs one below, at and one above the load at which the kernel gives the table up: the
    (cap / 2 + 1)-th claim sets the bail word.  Two root Maps share the pairs (a block holds MF_KMAX keys at most)."""
    groups = []
    n_rows = 3000 if ht_opt is None else 100
    half = table_cap(n_rows, ht_opt) // 2
    for n in (half - 1, half, half + 1):
        a, b = wire.Replica(21), wire.Replica(12)
        pairs = [("m%d" % (i % 2), "k%d" % (i // 2)) for i in range(n)]
        for i in range(n_rows):
            r = (a, b)[i * 2 // n_rows]
            name, key = pairs[i % n]
            r.map_set(name, key, i)
            if i % 500 == 499:
                r.commit()
        a.commit(); b.commit()
        d = MapDoc("%d distinct pairs, a table of %d" % (n, 2 * half), [a, b])      # (no checkout: a version claims slots for the pairs it holds only)
        assert sum(len(c.ops) for c in d.model.changes) == n_rows and table_cap(n_rows, ht_opt) == 2 * half
        groups.append(("%d pairs in a table of %d" % (n, 2 * half), STAYS, [d]))      # (entry_leaves decides: the side depends on the setting's LM_HT_OPT)
    return groups


def peer_ids(rng, n):
    """`n` distinct peer ids from the whole 64-bit range, in no order"""
    out = []
    while len(out) < n:
        p = rng.getrandbits(64)
        if p and p not in out:
            out.append(p)
    return out


EDGE_PEERS = [1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]


def peer_docs():
    docs = []
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [3, 5, 0, 4, 2, 1]):
        reps = [wire.Replica(EDGE_PEERS[i]) for i in order]
        for r in reps:
            r.map_set("m", "k", "from %d" % r.peer); r.map_set("m", "k%d" % (r.peer % 3), r.peer % 1000); r.commit()
        pairs = [[(a.peer, 0), (b.peer, 0)] for i, a in enumerate(reps) for b in reps[i + 1:]]
        d = MapDoc("a lamport tie between peer ids on both sides of 2^32 and 2^63, delivered %s" % order, reps, versions=[[(r.peer, 0)] for r in reps] + [sorted(p) for p in pairs])
        got = d.model.map_outcomes(d.delivery)
        assert got["tie_on_lamport"] == 3 and d.model.value()["m"]["k"] == "from %d" % ((1 << 64) - 1), got
        docs.append(d)
    rng = random.Random(200)
    reps = [wire.Replica(p) for p in peer_ids(rng, 200)]
    for r in reps:
        r.map_set("m", "k", r.peer % 100000); r.commit()
    docs.append(MapDoc("200 peers, one write each to one key at lamport 0", reps, versions=[[(reps[7].peer, 0)], [(reps[7].peer, 0), (reps[150].peer, 0)]]))
    assert docs[-1].model.value() == {"m": {"k": max(r.peer for r in reps) % 100000}}
    groups = [("peers", STAYS, docs)]
    for n in (LIMITS["MAX_PEERS"] - 1, LIMITS["MAX_PEERS"]):
        reps = [wire.Replica(p) for p in peer_ids(rng, n)]
        for r in reps:
            r.map_set("m", "k", r.peer % 100000); r.map_set("m", "k%d" % (r.peer % 5), 1); r.commit()
        groups.append(("%d peers" % n, STAYS if n < LIMITS["MAX_PEERS"] else "refused", [MapDoc("%d peers" % n, reps)]))
    return groups


def filter_docs():
    """the applied-change filter (ch_flag), the sliced-prefix filter (ch_skip) and the version filter, with pending changes"""
    docs = []
    a, b, c = wire.Replica(30), wire.Replica(20), wire.Replica(10)
    for i in range(20):
        a.map_set("m", "k%d" % (i % 6), i)
    for i in range(5):
        c.map_set("m", "c%d" % i, "c")
    sync(a, b, c)
    for i in range(20):
        b.map_set("m", "k%d" % (i % 7), "b%d" % i)
    b.commit()
    sync(a, b, c)
    for r in (a, c):
        for i in range(10):
            r.map_set("m", "k%d" % i, "%d:%d" % (r.peer, i))
        r.commit()
    own = {r.peer: r.changes[r.peer] for r in (a, b, c)}
    # (checkouts of the APPLIED part — a change end, inside a change, a two-peer frontier, nothing: the kernel's applied-change filter
    # together with its version filter; the pending count does not depend on the version)
    docs.append(MapDoc("a missing peer", [a, c], delivered=own[30] + own[10], changes=changes_of([a, b, c]),
                       versions=[[(30, 19)], [(30, 7)], [(10, 2), (30, 7)], [(10, 4)], [(10, 4), (30, 19)], []]))
    assert docs[-1].model.pending == 20 and docs[-1].model.value() == {"m": dict({"k%d" % (i % 6): i for i in range(14, 20)}, **{"c%d" % i: "c" for i in range(5)})}
    assert all(docs[-1].model.result(v)[3] == 20 for v in docs[-1].versions) and docs[-1].model.value([(30, 7)]) == {"m": {"k%d" % (i % 6): i for i in range(2, 8)}}
    # three incremental blobs of one peer, the second is missing
    p, q = wire.Replica(5), wire.Replica(6)
    parts, have = [], {}
    for rnd in range(3):
        for i in range(8):
            p.map_set("m", "k%d" % (i % 5), rnd * 100 + i)
            if i % 3 == 2:
                p.commit()
        p.commit()
        parts.append((p.export(dict(have)), [ch for ch in p.changes[5] if ch.counter >= have.get(5, 0)]))
        have = dict(p.vv)
    for i in range(6):
        q.map_set("m", "k%d" % i, "q")
    q.commit()
    docs.append(MapDoc("a blob missing from the middle of one peer's history", [p, q], blobs=[parts[0][0], parts[2][0], q.export()], delivered=parts[0][1] + parts[2][1] + q.changes[6],
                       versions=[[(5, 7)], [(5, 4)], [(5, 3), (6, 2)], [(6, 5)], []]))
    assert docs[-1].model.pending == 8 and all(docs[-1].model.result(v)[3] == 8 for v in docs[-1].versions)
    docs.append(MapDoc("the missing blob delivered last", [p, q], blobs=[parts[2][0], q.export(), parts[0][0], parts[1][0]], versions=[[(5, 11)], [(5, 20), (6, 2)]]))
    docs.append(MapDoc("an applied blob delivered twice", [p, q], blobs=[parts[0][0], q.export(), parts[0][0], parts[1][0], q.export(), parts[1][0], parts[2][0]], versions=[[(5, 11)]]))
    # overlapping exports of one history with different change boundaries: the second change is sliced on import
    cid = wire.root_cid("m", K.KIND_MAP)

    def ops(lo, hi):
        return [wire.Op(cid, i, "map_set", key="k%d" % (i % 4), value=i) if i % 5 else wire.Op(cid, i, "map_delete", key="k%d" % (i % 4)) for i in range(lo, hi)]
    c1, c2 = wire.Change(7, 0, 0, [], ops(0, 20)), wire.Change(7, 10, 10, [(7, 9)], ops(10, 31))
    tail = wire.Change(7, 20, 20, [(7, 19)], ops(20, 31))
    other = wire.Replica(9)
    for i in range(25):
        other.map_set("m", "k%d" % (i % 4), "o%d" % i)
    other.commit()
    for order in ((c1, c2), (c2, c1)):
        blobs = [wire.encode_updates([[x]]) for x in order] + [other.export()]
        docs.append(MapDoc("overlapping exports, the second change is sliced%s" % (", reversed" if order[0] is c2 else ""), [other], blobs=blobs,
                           changes=[c1, tail] + other.changes[9], delivered=[c1, c2] + other.changes[9], versions=[[(7, 15)], [(7, 25)], [(7, 19), (9, 20)]]))
        assert docs[-1].model.pending == 0
    return [("filters", STAYS, docs)]


def checkout_docs():
    """every change end, counters in the middle of a change, two-peer frontiers"""
    a, b, c = wire.Replica(1 << 33), wire.Replica(4), wire.Replica(77)
    rng = random.Random(9)
    for rnd in range(4):
        for r in (a, b, c):
            for i in range(rng.randint(3, 9)):
                if rng.random() < 0.2:
                    r.map_delete("m", "k%d" % rng.randrange(5))
                else:
                    r.map_set("m", "k%d" % rng.randrange(5), scalar(rng))
            r.commit()
        if rnd % 2:
            sync(a, b, c)
    reps = [a, b, c]
    vs = ends_of(reps)
    vs += [[(r.peer, k)] for r in reps for ch in r.changes[r.peer] for k in range(ch.counter, ch.ctr_end - 1)][::2]
    vs += [sorted([(a.peer, i), (b.peer, j)]) for i in range(0, a.vv[a.peer], 4) for j in range(1, b.vv[b.peer], 5)] + [[]]
    return [("checkouts", STAYS, [MapDoc("three peers at %d versions" % len(vs), reps, versions=vs)])]


def race_docs():
    """GPU only.  32 and 65 blocks of 1,024 rows each, written by 16 peers (every peer starts at lamport 0, so every row's lamport is
    shared by 16 writes) onto 1, 2, 4 and 1,000 keys: 16 waves of one workgroup race for the same table slots — the CAS claim followed
    by the prefix store, a plain read of the maximum followed by the atomic maximum."""
    docs = []
    R = LIMITS["MF_RMAX"]
    for n_blocks in (32, 65):
        for n_keys in (1, 2, 4, 1000):
            reps = [wire.Replica(p) for p in peer_ids(random.Random(n_blocks * 7 + n_keys), 16)]
            blocks = []
            for bk in range(n_blocks):
                r = reps[bk % 16]
                for i in range(R):
                    r.map_set("m", "k%d" % ((i * 7 + bk // 16) % n_keys), bk * R + i)      # (the 16 blocks of a round: the same key at the same lamport)
                r.commit()
                blocks.append([r.changes[r.peer][-1]])
            blobs = [wire.encode_updates([bl for bl in blocks if bl[0].peer == r.peer]) for r in reps]
            docs.append(MapDoc("%d blocks of %d rows by 16 peers on %d keys" % (n_blocks, R, n_keys), reps, blobs=blobs))
            if n_blocks == 32:          # every key's winner ties with the 15 other peers of the last round (65 blocks end with one peer alone)
                assert docs[-1].model.map_outcomes()["tie_on_lamport"] == n_keys
    return [("races", STAYS, docs)]


def hand_built(ht_opt=None):
    """every CPU + GPU group; the table documents for the host's choice under `ht_opt`"""
    return key_docs() + column_docs() + value_docs() + row_docs() + table_docs(ht_opt) + peer_docs() + filter_docs() + checkout_docs()


# ---------------------------------------------------------------------------------------------------------------------- running
# the five settings both test modules run under: (name, environment, is k_map_fused on, LM_HT_OPT).  lm_pipeline.h `mf_on`: the fused
# kernel needs LM_MAP_FUSED, the LDS LWW kernels and an optimistic table of at most LWW_LDS_CAP slots; the decoder choice does not touch it
SETTINGS = [("fused", dict(FORCE), True, None), ("LM_MAP_FUSED=0", dict(FORCE, LM_MAP_FUSED="0"), False, None), ("LM_LWW_LDS=0", dict(FORCE, LM_LWW_LDS="0"), False, None),
            ("LM_HT_OPT=64", dict(FORCE, LM_HT_OPT="64"), True, 64), ("LM_DECODE=0", dict(FORCE, LM_DECODE="0"), True, None)]


def n_renderings(groups):
    """every document of every group at the latest version and at each of its versions: what a run over the groups must have compared"""
    return sum(1 + len(d.versions) for _, _, docs in groups for d in docs)


def entry_leaves(path, d, fr, ht_opt=None):
    """does k_map_fused hand this entry over?  Its group says so, or the version holds more distinct (Map, key) pairs than half the
    largest table the host gives a document (a smaller table is sized for twice the document's rows and cannot fill up)"""
    return path == LEAVES or d.model.map_pairs(fr) > (ht_opt if ht_opt is not None else LIMITS["LWW_LDS_CAP"]) // 2


def run_group(ctx, label, path, docs, oracle=None, what="", repeat=1, max_versions=None, fused_on=True, ht_opt=None):
    """`docs` at the latest version and at their versions, one batch on `ctx` (a harness Context or the device's MergeEngine): every
    result against the model's, and the batch's fused / redo counts EXACTLY against the group's path (`fused_on`: whether the
    settings leave k_map_fused on at all).  Returns the number of renderings."""
    at = [(d, None) for d in docs] + [(d, fr) for d in docs for fr in d.versions[:max_versions]]
    at = at * repeat
    blobs = [d.blobs for d, _ in at]
    fronts = [None if fr is None else wire.encode_frontiers(fr) for _, fr in at]
    got = ctx.merge_batch(blobs, fronts)
    counts = (ctx.b.fused_documents(ctx.h), ctx.b.redo_documents(ctx.h))
    assert len(got) == len(at)
    if path == "refused":       # one peer more than k_doc_tables takes: a status, not a rendering
        assert all(g[0] != 0 and g[1] == b"" for g in got), (label, what, [g[:2] for g in got])
        want = (len(at), len(at)) if fused_on else (0, 0)
    else:
        for (d, fr), b, f, g in zip(at, blobs, fronts, got):
            w = d.model.result(fr)
            if g != w:
                third = oracle(b, f)[:3] if oracle else None
                raise AssertionError("%s %s %s at %s:\n device %r\n model  %r\n oracle %r" % (what, label, d.label, fr, g[:3], w[:3], third))
        want = (0, 0) if not fused_on or path == ROWS else (len(at), sum(1 for d, fr in at if entry_leaves(path, d, fr, ht_opt)))
    assert counts == want, "%s %s (%s): fused_documents, redo_documents = %r, expected %r" % (what, label, path, counts, want)
    return len(at)


