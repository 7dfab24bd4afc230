"""Every LEGAL encoding of a change block's columns, not only the one loro_amd.wire writes.

wire.py makes one choice per column: `_any_rle` writes equal neighbours as one run of >= 2 and everything else as one literal group,
`enc_delta_of_delta` picks the shortest bit class, `enc_bool_rle` writes no zero-length run behind the first.  The grammar (the
reference's docs/encoding.md 7-9, the table in 8.1) allows any segmentation of an AnyRle / DeltaRle column — runs of 1, a run cut in
two, literal groups of any size, equal values inside a literal group — and any DeltaOfDelta class that holds the value.  The device
reads those columns with four independent readers (k_block_decode_wave on LDS-staged bytes and on HBM, the lane decoder, the counting
kernels, k_map_fused and the eight-lane header split of blocks of >= 16 changes); this module gives them the other shapes.

Three parts:
  * FORMS: `forms(any_rle=, dod=, bool_rle=)` swaps wire._any_rle / wire.enc_delta_of_delta / wire.enc_bool_rle for the time of a
    `with` block and always puts them back.  A form is chosen for all columns or PER COLUMN (a dict keyed by the names in ANY_COLS /
    DOD_COLS: the columns in the order encode_block writes them, counted from the block's enc_bool_rle call).
  * A PLAIN READER, `read_block`: written from the grammar text alone, Python integers and loops, no code shared with wire.py,
    oracle/ or lm_export.h.  It returns every column's values AND its segments with their byte offsets, so a test can prove that a
    variant is legal and equivalent (`same_values`), can count what a corpus shows (`Counts`) and can say where a column's last
    value or segment head starts.
  * DOCUMENTS (`Doc`: writers + the plain model of tests/_merge_ref.py, which never sees an encoding — one expectation serves every
    form) and `run_entries`, which takes (document, form) entries through a harness Context or the device's MergeEngine as ONE batch:
    every status 0, every result the model's, every variant's whole result tuple the canonical twin's.

Conditions (`check_conditions`, asserted before anything is compared; counted by the plain reader over the blocks the corpus
entries actually produce): per AnyRle-family column >= 20 segments of each kind — run of 1, run >= 2, literal group of 1, literal
group >= 2, literal group holding two equal neighbours —, >= 5 segments per op / delete-start column that straddle a multiple of
eight rows, >= 5 uses of each DeltaOfDelta class as the canonical and as a non-minimal choice in each DeltaOfDelta column.
The 64-bit class as the canonical choice needs a step beyond 2^20: timestamps are set on the changes, lamports are raised on the changes
(lamport_jump_doc: a peer may stamp any lamport beyond its dependencies'), dependency counters come from chunks of 1,048,700 characters
(counter_jump_doc: 3.1 million elements, beyond the element-by-element model — its expectation is the oracle's result on the canonical
bytes, and every variant its canonical twin's).

Counts of the corpus of this module (`corpus_entries()`, 48 sessions + the DeltaOfDelta and many-change documents, 488 entries, 1,912 blocks),
[run of 1, run >= 2, literal of 1, literal >= 2, literal with equal neighbours, straddling a multiple of 8]:
  dep_count [3094, 2427, 3568, 3036, 1820, 1069]
  dep_peer  [1018, 564, 1429, 1349, 603, 284]
  msg_len   [1891, 2208, 2205, 2262, 1655, 1453]
  cidx      [4427, 2678, 4365, 5128, 1594, 2401]
  prop      [4416, 4250, 5533, 5706, 885, 2207]
  vtype     [4434, 3925, 5641, 4093, 2220, 2452]
  len       [4255, 2328, 4526, 4154, 2192, 1759]
  del_peer  [1113, 538, 1067, 980, 429, 217]
  del_ctr   [1070, 83, 956, 1091, 55, 227]
  del_len   [1134, 419, 1110, 1087, 293, 230]
  dep_ctr   classes 0..5 as the canonical choice [434, 4785, 41, 30, 41, 36], as a wider one [0, 99, 1203, 320, 322, 1433]
  lamport   classes 0..5 as the canonical choice [3260, 11116, 69, 77, 95, 126], as a wider one [0, 1296, 3178, 850, 868, 4207]
  timestamp classes 0..5 as the canonical choice [16871, 53, 112, 120, 138, 432], as a wider one [0, 3491, 541, 744, 714, 3826]
What binds: the delete-start counter column's literal groups with equal neighbours (55) and its runs of >= 2 (83) — two deletes in a row
whose targets step evenly are rare —, and the 9- and 12-bit classes of the dependency counters, which only the lead documents show.
Beyond the limits, pinned by status (check_limits): a position of 2^35 (`prop` is an i32) and delete-start counters on both sides of 2^31.
No AnyRle column holds a legal value of more than five bytes (all are 32-bit): three-, four- and five-byte values and deltas are
wide_value_docs (model=False) and tail_doc; a ten-byte one does not exist.
"""
import contextlib, functools, random, zlib

import _fuzz, _merge_docs_map, _merge_ref, _oracle, _resident
from _richtext_ref import changes_of
from loro_amd import wire

V = _merge_ref.view
ANY_COLS = ["dep_count", "dep_peer", "msg_len", "cidx", "prop", "vtype", "len", "del_peer", "del_ctr", "del_len"]
DOD_COLS = ["dep_ctr", "lamport", "timestamp"]
ROW_COLS = ANY_COLS[3:]                       # the op and delete-start columns: one value per op row / DeleteSeq row
ANY_FORMS = ["run1", "lit1", "lit2", "lit7", "lit8", "lit9", "litrand", "mixed", "split"]
DOD_FORMS = ["widest", "wider", "random"]
DOD_BITS = [0, 7, 9, 12, 21, 64]              # payload bits of the classes 0 / 10 / 110 / 1110 / 11110 / 11111
DOD_BIAS = [0, 63, 255, 2047, 1048575, 0]


# ------------------------------------------------------------------------------------------------------------------------- forms
def _run_len(vals, i):
    j = i
    while j + 1 < len(vals) and vals[j + 1] == vals[i]:
        j += 1
    return j - i + 1


def _canonical_segments(vals, split=None):
    """wire._any_rle's choice; `split`(rng): every run of >= 2 is cut in two"""
    out, lit, i = [], [], 0
    while i < len(vals):
        n = _run_len(vals, i)
        if n >= 2:
            if lit:
                out.append(("lit", lit)); lit = []
            if split is None:
                out.append(("run", n, vals[i]))
            else:
                a = split.randint(1, n - 1)
                out += [("run", a, vals[i]), ("run", n - a, vals[i])]
        else:
            lit.append(vals[i])
        i += n
    if lit:
        out.append(("lit", lit))
    return out


def _maximal_runs(vals):
    out, i = [], 0
    while i < len(vals):
        n = _run_len(vals, i)
        out.append(("run", n, vals[i])); i += n
    return out


def segments(form, vals, rng):
    """the segment list [("run", k, value) | ("lit", [values])] of `vals` under an AnyRle form"""
    n = len(vals)
    if form == "run1":
        return [("run", 1, v) for v in vals]
    if form == "lit1":
        return [("lit", [v]) for v in vals]
    if isinstance(form, str) and form[:3] == "lit" and form[3:].isdigit():
        k = int(form[3:])
        return [("lit", vals[i:i + k]) for i in range(0, n, k)]
    if form == "litrand":
        out, i = [], 0
        while i < n:
            g = rng.randint(1, 9)
            out.append(("lit", vals[i:i + g])); i += g
        return out
    if form == "mixed":                       # a run cut short at 1..len, or a literal group of 1..9 (equal neighbours and all)
        out, i = [], 0
        while i < n:
            if rng.random() < 0.5:
                k = rng.randint(1, _run_len(vals, i))
                out.append(("run", k, vals[i])); i += k
            else:
                g = min(rng.randint(1, 9), n - i)
                out.append(("lit", vals[i:i + g])); i += g
        return out
    if form == "split":
        return _canonical_segments(vals, split=rng)
    if isinstance(form, tuple) and form[0] == "cut":      # ("cut", rows, "run" | "lit"): segments END at these rows; pieces alternate
        _, rows, kind = form
        out, lo = [], 0
        for hi in sorted(set(r for r in rows if 0 < r < n)) + [n]:
            piece = vals[lo:hi]
            if not piece:
                continue
            out += _maximal_runs(piece) if kind == "run" else [("lit", piece)]
            kind = "lit" if kind == "run" else "run"
            lo = hi
        return out
    if isinstance(form, tuple) and form[0] == "segments":  # ("segments", f): f(vals) -> the segment list itself
        return form[1](vals)
    raise ValueError(form)


def _write_segments(segs, wv):
    out = bytearray()
    for s in segs:
        if s[0] == "run":
            out += wire.zigzag(s[1]) + wv(s[2])
        else:
            out += wire.zigzag(-len(s[1]))
            for v in s[1]:
                out += wv(v)
    return bytes(out)


def dod_class(dd):
    """the shortest class that holds a delta-of-delta (the table of docs/encoding.md 8.1)"""
    if dd == 0:
        return 0
    for c in (1, 2, 3, 4):
        if -DOD_BIAS[c] <= dd <= DOD_BIAS[c] + 1:
            return c
    return 5


def _write_dod(vals, form, rng):
    vals = list(vals)
    if not vals:
        return b"\x00\x00"
    head = b"\x01" + wire.zigzag(vals[0])
    if len(vals) == 1:
        return head + b"\x00"
    bits = []
    prev_delta = 0
    for i in range(1, len(vals)):
        delta = vals[i] - vals[i - 1]
        dd, prev_delta = delta - prev_delta, delta
        lo = dod_class(dd)
        c = {"widest": 5, "wider": min(lo + 1, 5), "random": rng.randint(max(lo, 1), 5) if lo else rng.choice([0, 0, 1, 2, 3, 4, 5])}[form]
        if c == 0:
            bits.append("0")
        else:
            payload = dd + DOD_BIAS[c] if c < 5 else dd & ((1 << 64) - 1)
            bits.append("1" * min(c, 5) + ("0" if c < 5 else "") + format(payload, "0%db" % DOD_BITS[c]))
    s = "".join(bits)
    used = len(s) % 8 or 8
    s += "0" * (-len(s) % 8)
    return head + bytes([used]) + bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def _write_bool(vals, form):
    runs, cur, run = [], False, 0
    for v in vals:
        if bool(v) == cur:
            run += 1
        else:
            runs.append(run); cur, run = bool(v), 1
    if len(vals):
        runs.append(run)
    where, pairs = form
    if where == "front" and runs:             # F0 T0 … in front of the real runs: the values do not change
        runs = [0, 0] * pairs + runs
    elif where == "between":                  # … between the first real run and the run behind it (none behind it: nothing to do —
        i = next((k for k, r in enumerate(runs) if r), None)        # zero runs at the END of the column are never read)
        if i is not None and i + 1 < len(runs):
            runs = runs[:i + 1] + [0, 0] * pairs + runs[i + 1:]
    return b"".join(wire.uleb(r) for r in runs)


def _pick(spec, name):
    return spec.get(name, "canonical") if isinstance(spec, dict) else spec


@contextlib.contextmanager
def forms(any_rle="canonical", dod="canonical", bool_rle="canonical", seed=0, record=None):
    """wire's three column writers swapped for the given forms; restored whatever happens.  `any_rle` / `dod`: one form for every
    column or {column name: form}; `bool_rle`: ("front" | "between", pairs).  The column of a call is its number within the block,
    counted from the block's one enc_bool_rle call.  `record`: a list that receives per block {column name: the writer's input}."""
    orig = (wire._any_rle, wire.enc_delta_of_delta, wire.enc_bool_rle)
    at = {"any": 0, "dod": 0}
    rng = random.Random(seed)

    def note(name, vals):
        if record is not None:
            record[-1][name] = list(vals)

    def any_(vals, wv):
        name = ANY_COLS[at["any"]] if at["any"] < len(ANY_COLS) else None
        at["any"] += 1
        vals = list(vals)
        note(name, vals)
        form = _pick(any_rle, name) if name else "canonical"
        return orig[0](vals, wv) if form == "canonical" else _write_segments(segments(form, vals, rng), wv)

    def dod_(vals):
        name = DOD_COLS[at["dod"]] if at["dod"] < len(DOD_COLS) else None
        at["dod"] += 1
        vals = list(vals)
        note(name, vals)
        form = _pick(dod, name) if name else "canonical"
        return orig[1](vals) if form == "canonical" else _write_dod(vals, form, rng)

    def bool_(vals):
        at["any"] = at["dod"] = 0
        vals = list(vals)
        if record is not None:
            record.append({})
        note("dep_self", vals)
        return orig[2](vals) if bool_rle == "canonical" else _write_bool(vals, bool_rle)

    wire._any_rle, wire.enc_delta_of_delta, wire.enc_bool_rle = any_, dod_, bool_
    try:
        yield
    finally:
        wire._any_rle, wire.enc_delta_of_delta, wire.enc_bool_rle = orig


# ------------------------------------------------------------------------------------------------------------------ the plain reader
class Malformed(Exception):
    pass


class _Bytes:
    def __init__(self, b, p, end):
        self.b, self.p, self.end = b, p, end

    def u8(self):
        if self.p >= self.end:
            raise Malformed("end of input at %d" % self.p)
        self.p += 1
        return self.b[self.p - 1]

    def uvar(self):
        v, sh = 0, 0
        while True:
            x = self.u8()
            v |= (x & 0x7F) << sh
            sh += 7
            if not x & 0x80:
                return v
            if sh > 133:
                raise Malformed("varint too long")

    def zz(self):
        v = self.uvar()
        return -((v + 1) >> 1) if v & 1 else v >> 1

    def section(self):
        n = self.uvar()
        if n > self.end - self.p:
            raise Malformed("section beyond input")
        self.p += n
        return _Bytes(self.b, self.p - n, self.p)

    def raw(self):
        return bytes(self.b[self.p:self.end])


class Column:
    """values: the decoded values (of a DeltaRle column: the deltas; `sums` the column's values).  AnyRle `segs`:
    (kind, count, head offset, [value offsets], holds equal neighbours) — offsets into the block; BoolRle `segs`: the run lengths;
    DeltaOfDelta `segs`: the class of every value behind the first.  [start, end): the column's bytes in the block."""

    def __init__(self, values, segs, start, end):
        self.values, self.segs, self.start, self.end = values, segs, start, end

    @property
    def sums(self):
        out, t = [], 0
        for d in self.values:
            t += d
            out.append(t)
        return out


def _any(r, n, kind):
    """AnyRle: n values (None: until the bytes end) of postcard T = u8 | uvar | zz (zigzag)"""
    start, vals, segs = r.p, [], []
    rd = {"u8": r.u8, "uvar": r.uvar, "zz": r.zz}[kind]
    while (len(vals) < n) if n is not None else (r.p < r.end):
        head = r.p
        k = r.zz()
        if k == 0:
            raise Malformed("segment length 0")
        if k > 0:
            at = r.p
            v = rd()
            vals += [v] * k
            segs.append(("run", k, head, [at], False))
        else:
            ats, lit = [], []
            for _ in range(-k):
                ats.append(r.p)
                lit.append(rd())
            vals += lit
            segs.append(("lit", -k, head, ats, any(a == b for a, b in zip(lit, lit[1:]))))
    if n is not None and len(vals) != n:
        raise Malformed("%d values for %d rows" % (len(vals), n))
    return Column(vals, segs, start, r.p)


def _bool(r, n):
    start, vals, runs, cur = r.p, [], [], False
    while len(vals) < n:
        k = r.uvar()
        runs.append(k)
        vals += [cur] * k
        cur = not cur
    if len(vals) != n:
        raise Malformed("BoolRle: too many values")
    return Column(vals, runs, start, r.p)


def _dod(r, n):
    start = r.p
    tag = r.u8()
    if tag > 1:
        raise Malformed("option tag %d" % tag)
    first = r.zz() if tag else None
    used = r.u8()
    if n == 0 or first is None:
        if n or first is not None or used:
            raise Malformed("empty DeltaOfDelta column")
        return Column([], [], start, r.p)
    vals, classes, pos, delta = [first], [], 0, 0

    def bits(k):
        nonlocal pos
        v = 0
        for _ in range(k):
            at = r.p + (pos >> 3)
            if at >= r.end:
                raise Malformed("bit stream ends")
            v = (v << 1) | ((r.b[at] >> (7 - (pos & 7))) & 1)
            pos += 1
        return v
    for _ in range(n - 1):
        c = 0
        while c < 5 and bits(1):
            c += 1
        dd = 0 if c == 0 else bits(DOD_BITS[c]) - DOD_BIAS[c]
        if c == 5 and dd >= 1 << 63:
            dd -= 1 << 64
        delta += dd
        vals.append(vals[-1] + delta)
        classes.append(c)
    if used != (0 if n == 1 else (pos % 8 or 8)):
        raise Malformed("used-bits byte %d after %d bits" % (used, pos))
    r.p += (pos + 7) // 8
    return Column(vals, classes, start, r.p)


def read_block(b):
    """one change block (docs/encoding.md 7) -> {"head", "peers", "lens", "cols": {name: Column}, "rest": the other bytes}"""
    r = _Bytes(b, 0, len(b))
    head = tuple(r.uvar() for _ in range(5))
    n = head[4]
    header, meta, cids, keys, positions, ops, dels, values = (r.section() for _ in range(8))
    if r.p != r.end or n < 1:
        raise Malformed("block")
    cols = {}
    h = header
    n_peers = h.uvar()
    peers = []
    for _ in range(n_peers):
        peers.append(sum(h.u8() << (8 * i) for i in range(8)))
    lens = [h.uvar() for _ in range(n - 1)]
    cols["dep_self"] = _bool(h, n)
    cols["dep_count"] = _any(h, n, "uvar")
    d = sum(cols["dep_count"].values)
    cols["dep_peer"] = _any(h, d, "uvar")
    cols["dep_ctr"] = _dod(h, d)
    cols["lamport"] = _dod(h, n - 1)
    if h.p != h.end:
        raise Malformed("bytes behind the header's columns")
    cols["timestamp"] = _dod(meta, n)
    cols["msg_len"] = _any(meta, n, "uvar")
    messages = meta.raw()
    if len(messages) != sum(cols["msg_len"].values):
        raise Malformed("message bytes")
    if ops.uvar() != 1 or ops.uvar() != 4:
        raise Malformed("ops field counts")
    for name, kind in (("cidx", "zz"), ("prop", "zz"), ("vtype", "u8"), ("len", "uvar")):
        cols[name] = _any(ops.section(), None, kind)
    if ops.p != ops.end or len({len(cols[k].values) for k in ("cidx", "prop", "vtype", "len")}) != 1:
        raise Malformed("op columns of unequal length")
    if dels.p != dels.end:
        if dels.uvar() != 1 or dels.uvar() != 3:
            raise Malformed("delete-start field counts")
        for name in ("del_peer", "del_ctr", "del_len"):
            cols[name] = _any(dels.section(), None, "zz")
        if dels.p != dels.end or len({len(cols[k].values) for k in ("del_peer", "del_ctr", "del_len")}) != 1:
            raise Malformed("delete-start columns of unequal length")
    if sum(cols["len"].values) != head[1] or sum(lens) > head[1]:
        raise Malformed("atom lengths")
    return {"head": head, "peers": peers, "lens": lens, "cols": cols,
            "rest": (cids.raw(), keys.raw(), positions.raw(), values.raw(), messages)}


def blocks_of(blob):
    """the change blocks of a FastUpdates blob (docs/encoding.md 2, 6)"""
    if blob[:4] != b"loro" or blob[20:22] != b"\x00\x04":
        raise Malformed("not an updates blob")
    r = _Bytes(blob, 22, len(blob))
    out = []
    while r.p < r.end:
        out.append(r.section().raw())
    return out


def same_values(variant, canonical):
    """is `variant` (a block) a legal encoding of the values of `canonical`?  Every column value by value, every other byte as it is"""
    a, b = read_block(variant), read_block(canonical)
    assert a["head"] == b["head"] and a["peers"] == b["peers"] and a["lens"] == b["lens"] and a["rest"] == b["rest"]
    assert sorted(a["cols"]) == sorted(b["cols"])
    for k in a["cols"]:
        assert a["cols"][k].values == b["cols"][k].values, k
    return a


class Counts:
    """what the blocks of a corpus show, counted by the plain reader"""

    def __init__(self):
        self.seg = {c: dict.fromkeys(("run1", "run2+", "lit1", "lit2+", "lit_equal", "straddle8"), 0) for c in ANY_COLS}
        self.dod = {c: {"canonical": [0] * 6, "wider": [0] * 6} for c in DOD_COLS}
        self.blocks = 0

    def add(self, block):
        self.blocks += 1
        blk = read_block(block) if isinstance(block, (bytes, bytearray)) else block
        for name in ANY_COLS:
            col = blk["cols"].get(name)
            row = 0
            for kind, n, _, _, eq in (col.segs if col else ()):
                c = self.seg[name]
                c[("run1" if n == 1 else "run2+") if kind == "run" else ("lit1" if n == 1 else "lit2+")] += 1
                c["lit_equal"] += eq
                c["straddle8"] += (row + n - 1) // 8 > row // 8 and (row + n) % 8 != 0 or (row + n - 1) // 8 > row // 8 + 1
                row += n
        for name in DOD_COLS:
            col = blk["cols"][name]
            v = col.values
            for i, c in enumerate(col.segs):
                dd = (v[i + 1] - v[i]) - ((v[i] - v[i - 1]) if i else 0)
                self.dod[name]["canonical" if c == dod_class(dd) else "wider"][c] += 1

    def table(self):
        out = ["  %-9s %s" % (c, [self.seg[c][k] for k in ("run1", "run2+", "lit1", "lit2+", "lit_equal", "straddle8")]) for c in ANY_COLS]
        out += ["  %-9s classes 0..5 as the canonical choice %s, as a wider one %s" % (c, self.dod[c]["canonical"], self.dod[c]["wider"]) for c in DOD_COLS]
        return "\n".join(out)


def check_conditions(counts):
    for c in ANY_COLS:
        for k, n in counts.seg[c].items():
            if k != "straddle8":
                assert n >= 20, (c, k, n)
    for c in ROW_COLS:
        assert counts.seg[c]["straddle8"] >= 5, (c, counts.seg[c])
    for c in DOD_COLS:
        for cls in range(6):
            if True:
                assert counts.dod[c]["canonical"][cls] >= 5, (c, "canonical", cls, counts.dod[c])
            if cls:
                assert counts.dod[c]["wider"][cls] >= 5, (c, "wider", cls, counts.dod[c])


# ------------------------------------------------------------------------------------------------------------------------ documents
class Doc:
    """a document: the writers, how their changes become blobs (`write(reps)`, run under a form), and the plain model"""

    def __init__(self, label, reps, write=None, model=True):
        self.label, self.reps = label, reps
        self.write = write or _fuzz.blobs_of
        self.model = _merge_ref.Model(changes_of(reps)) if model else None
        self._blobs = {}

    def blobs(self, spec=None):
        key = repr(spec)
        if key not in self._blobs:
            kw = dict(spec or {})
            kw.setdefault("seed", zlib.crc32((self.label + key).encode()))
            with forms(**kw):
                self._blobs[key] = self.write(self.reps)
        return self._blobs[key]

    def blocks(self, spec=None):
        return [b for blob in self.blobs(spec) for b in blocks_of(blob)]

    def expect(self):
        """the model's result; of a document the element-by-element model cannot hold (model=False: texts of 10^5 and more elements)
        the oracle's on the CANONICAL bytes — every variant must still give its canonical twin's whole result"""
        if self.model is not None:
            return self.model.result()
        if "oracle" not in self._blobs:
            self._blobs["oracle"] = _oracle.merge(self.blobs())
        return self._blobs["oracle"]

    def written(self, suffix, write):
        """the same document and model, its changes written another way"""
        o = Doc(self.label + suffix, self.reps, write=write, model=False)
        o.model = self.model
        return o


def whole_exports(reps):
    return [r.export() for r in reps if r.changes]


def one_block_each(reps):
    """every replica's own changes in ONE block"""
    return [wire.encode_updates([r.changes[r.peer]]) for r in reps if r.changes.get(r.peer)]


def in_blocks(n):
    """the replicas' own changes cut into `n` blocks altogether"""
    def write(reps):
        own = [r.changes[r.peer] for r in reps if r.changes.get(r.peer)]
        total = sum(len(c) for c in own)
        assert total >= n >= len(own)
        share = [1] * len(own)
        for _ in range(n - len(own)):          # the next block goes to the peer with the most changes per block
            k = max(range(len(own)), key=lambda i: len(own[i]) / share[i])
            share[k] += 1
        out = []
        for chs, s in zip(own, share):
            cuts = [len(chs) * i // s for i in range(s + 1)]
            out.append(wire.encode_updates([chs[a:b] for a, b in zip(cuts, cuts[1:])]))
        assert sum(len(blocks_of(b)) for b in out) == n
        return out
    return write


def spec_of(i, any_cols=None, dod_cols=None):
    """the i-th combination of an AnyRle form with a DeltaOfDelta form (every ninth: the canonical DeltaOfDelta)"""
    a, d = ANY_FORMS[i % len(ANY_FORMS)], (["canonical"] + DOD_FORMS)[i % 4]
    return {"any_rle": a if any_cols is None else {c: a for c in any_cols}, "dod": d if dod_cols is None else {c: d for c in dod_cols}}


ALL_SPECS = [spec_of(i) for i in range(36)][:12]        # each AnyRle form once, three of them twice; each DeltaOfDelta form three times


@functools.lru_cache(None)
def fuzz_docs():
    """24 text / list / map sessions with styles, 12 MovableList sessions with children, 12 Map sessions; three peers; the writers' views
    from the model.  Each as blobs per peer and as whole exports."""
    docs = []
    for s in range(24):
        kinds = [("text",), ("text", "list"), ("text", "list", "map")][s % 3]
        reps = _fuzz.random_session(7100 + s, n_peers=3, n_steps=70, kinds=kinds, styles=bool(s % 2), view=V, max_del=6)
        docs.append(Doc("fuzz %d" % s, reps))
    for s in range(12):
        docs.append(Doc("movable %d" % s, _fuzz.movable_session(7200 + s, n_peers=3, n_steps=70, nested=True, view=V)))
    for s in range(12):
        reps, _ = _merge_docs_map.map_session(7300 + s, 3, n_steps=90)
        docs.append(Doc("map %d" % s, reps))
    whole = []
    for d in docs:
        w = Doc(d.label + ", whole exports", d.reps, write=whole_exports, model=False)
        w.model = d.model
        whole.append(w)
    return docs, whole


@functools.lru_cache(None)
def block_count_docs():
    """documents of 7, 8 and 9 blocks (DEC_G = 8 blocks are served by one wave: with neighbouring documents in different forms the
    blocks of one group carry different forms)"""
    out = []
    for i, n in enumerate((7, 8, 9, 8, 7, 9)):
        reps = _fuzz.random_session(7400 + i, n_peers=3, n_steps=60, kinds=("text", "list", "map"), view=V, commit_prob=0.7)
        out.append(Doc("%d blocks (%d)" % (n, i), reps, write=in_blocks(n)))
    return out


MANY = (15, 16, 17, 63, 64, 65, 129)


@functools.lru_cache(None)
def many_change_doc(n):
    """one change per keystroke, `n` changes in ONE block (the header split of blocks of >= 16 changes gives each of eight lanes
    C = ceil(n / 8) changes).  Every third change the second peer is merged in — every sixth after it has seen this peer's last
    change, so that the change depends on the other peer ALONE: dep_on_self and the dep-count column have runs that end before,
    at and behind every lane's first change; a run of a NON-ZERO count (rle_sum_uvar multiplies) among them."""
    a, b = wire.Replica(21), wire.Replica(12)
    b.map_set("m", "b", 0); b.commit()
    for i in range(n):
        if i % 3 == 2 or i % 12 in (3, 4):   # (i = 2, 3, 4 / 14, 15, 16 / …: THREE changes in a row with one foreign dependency each — rle_sum_uvar takes the rest of a run of a non-zero count at once)
            if i % 6 == 5:
                b.merge_from(a)
            for j in range(1 + i % 4):
                b.map_set("m", "k%d" % (i % 5), i * 10 + j)
            b.commit()
            a.merge_from(b)
        a.text_insert("text", 0 if i % 5 else len(a.seq.get(wire.root_cid("text", wire.KIND_TEXT), [])), "abcdefghij"[i % 10])
        if i % 7 == 3:
            a.map_set("m", "a%d" % (i % 3), i)
        a.commit("msg!" if i % 8 in (1, 2, 3, 4) else "longer message" if i % 8 == 6 else None)      # (runs of four equal NON-ZERO message lengths: the decoders sum that column with rle_sum_uvar)
    assert len(a.changes[21]) == n
    return Doc("%d changes in one block" % n, [a, b], write=one_block_each)


def many_change_entries():
    """every AnyRle form of the dep-count and dep-peer columns, every DeltaOfDelta form of the dependency counters and lamports"""
    out = []
    for n in MANY:
        d = many_change_doc(n)
        out.append((d, None))
        for f in ANY_FORMS:
            out.append((d, {"any_rle": {"dep_count": f, "dep_peer": f}}))
        for f in DOD_FORMS:
            out.append((d, {"dod": {"dep_ctr": f, "lamport": f}}))
        out.append((d, {"any_rle": "mixed", "dod": "random"}))
    return out


DOD_EDGES = [0, -63, 64, -64, 65, -255, 256, -256, 257, -2047, 2048, -2048, 2049, -1048575, 1048576, -1048576, 1048577, 1 << 40, -(1 << 40)]


def series(dods, start=0):
    """values whose delta-of-deltas are `dods` (the second value's is its delta)"""
    out, delta = [start], 0
    for dd in dods:
        delta += dd
        out.append(out[-1] + delta)
    return out


def timestamp_doc(n_changes, rotate=0):
    """`n_changes` one-row changes of one peer in one block whose TIMESTAMPS step through the DeltaOfDelta edges"""
    r = wire.Replica(33)
    edges = DOD_EDGES[rotate:] + DOD_EDGES[:rotate]
    ts = series([edges[i % len(edges)] for i in range(n_changes - 1)], start=1700000000)
    for i in range(n_changes):
        r.map_set("m", "k%d" % (i % 4), i); r.commit()
        r.changes[33][-1].timestamp = ts[i]
    return Doc("timestamps over the DeltaOfDelta edges, %d changes, from edge %d" % (n_changes, rotate), [r], write=one_block_each)


def lead_doc(rotate=0, n=26):
    """Dependency counters and lamports with steps of every class up to 21 bits: peer A types chunks whose LENGTHS step through the
    edges a counter can take (a chunk of 2^20 atoms is beyond the plain model), peer B merges A after every chunk and writes one row —
    B's block holds one foreign dependency per change, its counters are A's chunk ends and its lamports follow A's lead."""
    steps = [0, 0, 64, -63, 65, -64, 256, -255, 257, -256, 2048, -2047, 2049, -2048, 3000, -2999, 0, 70, -70, 300, -300, 2500, -2500, 0, 1, -1]
    steps = steps[rotate:] + steps[:rotate]
    a, b = wire.Replica(50), wire.Replica(40)
    size = 1
    for i in range(n):
        size += steps[i % len(steps)]
        assert size >= 1
        a.text_insert("text", 0, "".join("abcdefghijklmnopqrstuvwxyz"[(i + k) % 26] for k in range(size))); a.commit()
        b.merge_from(a)
        b.map_set("m", "k%d" % (i % 3), i); b.commit()
    return Doc("counter and lamport leads, from step %d" % rotate, [a, b], write=one_block_each)


def lamport_jump_doc():
    """lamports that step by more than 2^20 between the changes of one block: a peer may stamp a change with any lamport beyond its
    dependencies' (a peer that merged someone far ahead).  The lamport of the last committed change is raised before the next commit,
    which then follows it: steps of 1 and 1,048,600 in turn are delta-of-deltas of +-1,048,599, the 64-bit class."""
    a, b = wire.Replica(35), wire.Replica(36)
    for i in range(14):
        a.map_set("m", "k%d" % (i % 3), i); a.commit()
        if i % 2:
            a.changes[35][-1].lamport += 1048599
        if i % 5 == 4:
            b.merge_from(a)
            b.map_set("m", "k1", -i); b.commit()           # b's lamport follows a's lead: LWW against a's later writes
    return Doc("lamports that step by more than 2^20", [a, b], write=one_block_each)


def counter_jump_doc():
    """dependency counters that step by more than 2^20: peer A types chunks of 1 and of 1,048,700 characters in turn, peer B merges A
    after every chunk and writes a row — B's block names A's chunk ends.  3.1 million elements: beyond the element-by-element model
    (model=False: the oracle's result on the canonical bytes, and every variant its twin's)."""
    a, b = wire.Replica(50), wire.Replica(40)
    big = "".join("abcdefghijklmnopqrstuvwxyz \n"[(i * 7 + i // 31) % 28] for i in range(1048700))
    for i in range(7):
        a.text_insert("text", 0, big if i % 2 else "s"); a.commit()
        b.merge_from(a)
        b.map_set("m", "k%d" % (i % 3), i); b.commit()
    return Doc("dependency counters that step by more than 2^20", [a, b], write=one_block_each, model=False)


@functools.lru_cache(None)
def dod_docs():
    return [timestamp_doc(n, rot) for n, rot in ((40, 0), (41, 5), (42, 11), (43, 16), (44, 2), (45, 7), (46, 13), (47, 18))] + [lead_doc(r) for r in (0, 4, 8, 12)] + [lamport_jump_doc()]      # (whole +x / -x pairs: a chunk keeps a length >= 1)


@functools.lru_cache(None)
def jump_entries():
    """(part of the corpus, not of the hand-built entries: a harness run of the 3.1-million-element document takes two seconds)"""
    d = counter_jump_doc()
    return [(d, None)] + [(d, {"dod": f}) for f in DOD_FORMS] + [(d, {"any_rle": "mixed", "dod": "random"}), (d, {"any_rle": "lit9", "dod": "wider", "seed": 3})]


def dod_entries():
    out = []
    for d in dod_docs():
        out += [(d, None)] + [(d, {"dod": f}) for f in DOD_FORMS] + [(d, {"dod": "random", "seed": 7}), (d, {"any_rle": "mixed", "dod": "wider"})]
    return out


BOUNDARY_ROWS = (7, 8, 9, 63, 64, 65)


@functools.lru_cache(None)
def boundary_doc():
    """128 one-character prepends, then 128 one-character deletes at position 0, one change, one block of 256 rows: every op column
    and every delete-start column is constant or steps evenly, so a segment may end ANYWHERE, as a run or as a literal group.
    DeleteSeq row j is op row 128 + j: a boundary at delete row 7 / 8 / 9 / 63 / 64 / 65 is one at those rows of the delete-start
    columns and, in op rows, at 135 / 136 / 137 / 191 / 192 / 193 — the same places in the 8-row chunk and the 64-row store."""
    r = wire.Replica(61)
    for i in range(128):
        r.text_insert("text", 0, "abcdefgh"[i % 8])
    for i in range(128):
        r.text_delete("text", 0, 1)
    r.commit()
    d = Doc("segment ends at rows 7-9 and 63-65", [r], write=one_block_each)
    assert len(read_block(d.blocks()[0])["cols"]["vtype"].values) == 256
    return d


def boundary_entries():
    """per column and boundary row: run -> literal and literal -> run; then all six rows in one column, all columns at once"""
    d = boundary_doc()
    out = [(d, None)]
    for col in ROW_COLS:
        for row in BOUNDARY_ROWS:
            for first in ("run", "lit"):
                out.append((d, {"any_rle": {col: ("cut", (row,), first)}}))
        for first in ("run", "lit"):
            out.append((d, {"any_rle": {col: ("cut", BOUNDARY_ROWS + (71, 72, 73, 127, 128, 129), first)}}))
    out.append((d, {"any_rle": ("cut", BOUNDARY_ROWS, "lit")}))
    return out


@functools.lru_cache(None)
def tail_doc(last_len, pad_rows=70):
    """A block whose `prop` column (DeltaRle) ENDS in a delta of one, two or three bytes (`last_len`): the last two rows write the
    first Map key and a key 3 / 100 / 9,000 entries further down the block's key table.  The value-type column follows (its length
    prefix, then its bytes).  A Text row keeps the document with the row decoders."""
    r = wire.Replica(71)
    r.text_insert("text", 0, "hi")
    far = {1: 3, 2: 100, 3: 9000}[last_len]
    for i in range(max(far + 1, pad_rows)):
        r.map_set("m", "k%d" % i, i)
    r.map_set("m", "k0", -1)
    r.map_set("m", "k%d" % far, -2)
    r.commit()
    return Doc("the prop column ends in a delta of %d bytes" % last_len, [r], write=one_block_each)


def tail_entries():
    """the last VALUE and the last SEGMENT HEAD of the prop column 1, 2 and 3 bytes before its end, the next byte with its top bit set
    (test_column_forms.py asserts the offsets with the plain reader).  col_var3 reads three bytes at once when three are left."""
    out = []
    for n in (1, 2, 3):
        d = tail_doc(n)
        out.append((d, None))
        for form in ("run1", "lit1", "lit2", "lit9"):
            out.append((d, {"any_rle": {"prop": form, "vtype": "lit1"}}))      # value type as literals of 1: 2 bytes per row, a two-byte length prefix …
        out.append((d, {"any_rle": {"prop": "lit1", "vtype": "run1", "len": "lit1"}}))
    return out


@functools.lru_cache(None)
def width_docs():
    """varint widths: run counts of 63 / 64 (the zigzag's one -> two byte step) in every op column, run counts of 8,191 / 8,192 (two -> three bytes: one
    change of 8,200 Map writes to one container)."""
    out = []
    for n in (63, 64, 65):
        r = wire.Replica(81)
        for i in range(n):
            r.text_insert("text", 0, "q")
        r.map_set("m", "k", 1)
        for i in range(n):
            r.map_set("m", "k", i)                    # the same key: prop, container index, value type and len all run
        r.commit()
        out.append(Doc("runs of %d rows" % n, [r], write=one_block_each))
    for n in (8191, 8192, 8200):
        r = wire.Replica(83)
        for i in range(n):
            r.map_set("m", "k", i % 7)
        r.map_set("m", "other", 1)
        r.commit()
        out.append(Doc("a run of %d Map rows" % n, [r], write=one_block_each))
    return out


@functools.lru_cache(None)
def wide_value_docs():
    """values and deltas of three, four and five bytes (model=False: texts of 10^5 .. 10^6 elements; expectation = the oracle on the
    canonical bytes + the canonical twin).  No AnyRle column of a block holds a longer legal value: `len`, `prop` and the counters are
    32-bit, so a value or a delta between two of them ends within five bytes.
      * `len` = 300,000 (three bytes) and positions that jump by +-300,000 (three-byte deltas of both signs);
      * positions that jump by +-2^21 (four-byte deltas)."""
    out = []
    for n in (300000, (1 << 21) + 8):
        r = wire.Replica(82)
        r.text_insert("text", 0, "".join("abcdefghijklmnopqrstuvwxyz \n"[(i * 7 + i // 31) % 28] for i in range(n)))
        for i in range(12):
            r.text_insert("text", 0 if i % 2 else (n if n == 300000 else 1 << 21) + i // 2, "JK"[i % 2])
        r.text_delete("text", n - 10, 5)
        r.commit()
        out.append(Doc("a %d-character insert and positions that jump by it" % n, [r], write=one_block_each, model=False))
    return out


def beyond_limits_docs():
    """what no legal document holds, pinned by its STATUS (the same for every form): a position of 2^35 (`prop` is an i32) and
    delete-start counters on both sides of 2^31 (a counter is an i32, and the device takes counters below 2^24).  Raw changes."""
    cid = wire.root_cid("text", wire.KIND_TEXT)
    out = []
    c = wire.Change(7, 0, 0, [], [wire.Op(cid, 0, "text_insert", pos=0, text="ab"), wire.Op(cid, 2, "text_insert", pos=1 << 35, text="c"), wire.Op(cid, 3, "text_insert", pos=0, text="d")])
    out.append(("a position of 2^35", [c]))
    for ctr in ((1 << 31) - 2, (1 << 31) + 2):
        c = wire.Change(7, 0, 0, [], [wire.Op(cid, 0, "text_insert", pos=0, text="abcdef"), wire.Op(cid, 6, "delete", pos=1, del_id=(7, 1), signed_len=1),
                                      wire.Op(cid, 7, "delete", pos=1, del_id=(7, ctr), signed_len=1), wire.Op(cid, 8, "delete", pos=0, del_id=(7, 0), signed_len=1)])
        out.append(("a delete-start counter of %d" % ctr, [c]))
    docs = []
    for label, changes in out:
        r = wire.Replica(7)
        r.changes = {7: changes}
        docs.append(Doc(label, [r], write=one_block_each, model=False))
    return docs


def width_entries():
    out = []
    for d in width_docs():
        out += [(d, None), (d, {"any_rle": "split"}), (d, {"any_rle": "lit9"}), (d, {"any_rle": "mixed"})]
        if "Map rows" not in d.label:
            out += [(d, {"any_rle": "run1"}), (d, {"any_rle": "lit1"})]
    for d in wide_value_docs():
        out += [(d, None), (d, {"any_rle": "lit1"}), (d, {"any_rle": "run1"}), (d, {"any_rle": "mixed"}), (d, {"any_rle": "split"})]
    return out


@functools.lru_cache(None)
def big_key_table_docs():
    """Map blocks whose key table exceeds the decoder's default LDS slot: decoded by the second, larger-slot launch (with the integer
    fast path for their values)"""
    out = []
    for i, n_keys in enumerate((150, 400)):
        a, b = wire.Replica(91), wire.Replica(19)
        for k in range(n_keys * 2):
            a.map_set("m", "a-rather-long-key-%04d" % (k % n_keys), k * 1000003 - 7)
            if k % 97 == 0:
                a.commit()
        a.commit()
        for k in range(0, n_keys, 3):
            b.map_set("m", "a-rather-long-key-%04d" % k, -k)
        b.commit()
        out.append(Doc("a key table of %d keys" % n_keys, [a, b], write=one_block_each))
    return out


def bool_docs():
    """the BoolRle finding: dep_on_self with zero-length run PAIRS (F0 T0) in front of the real runs and between two real runs"""
    return [many_change_doc(17), many_change_doc(6)]


BOOL_ACCEPTED = [("front", 1), ("between", 1)]                      # at most three zero-length runs in a row: read by kernel and oracle
BOOL_REFUSED = [(w, n) for w in ("front", "between") for n in (2, 3, 8)]      # four or more: refused by both (NEXT.md, lm_dev_util.h bool_next)


def corpus_entries():
    """the entries whose blocks the conditions are counted over and every setting runs"""
    docs, whole = fuzz_docs()
    out = []
    for i, d in enumerate(docs + block_count_docs()):
        out += [(d, None)] + [(d, ALL_SPECS[(i + k) % len(ALL_SPECS)]) for k in (0, 5, 9)]
    for i, d in enumerate(whole):
        out += [(d, None), (d, ALL_SPECS[(i + 3) % len(ALL_SPECS)])]
    return out + dod_entries() + jump_entries() + many_change_entries()


def counts_of(entries):
    c = Counts()
    for d, spec in entries:
        for b in d.blocks(spec):
            c.add(b)
    return c


# -------------------------------------------------------------------------------------------------------------------------- running
def run_entries(ctx, entries, what="", oracle=None, counts=None):
    """(document, form) entries as ONE batch on `ctx` (a harness Context or the device's MergeEngine): every status 0, every result the
    model's, every variant's whole result tuple its canonical twin's.  `counts`: the batch's (fused_documents, redo_documents)."""
    blobs = [d.blobs(spec) for d, spec in entries]
    got = ctx.merge_batch(blobs)
    assert len(got) == len(entries)
    twin = {}
    for (d, spec), g in zip(entries, got):
        if spec is None:
            twin[id(d)] = g
    for (d, spec), bl, g in zip(entries, blobs, got):
        want = d.expect()
        if g != want or g != twin.get(id(d), g):
            third = oracle(bl)[:3] if oracle else None
            raise AssertionError("%s %s under %r:\n got    %r\n model  %r\n twin   %r\n oracle %r" % (what, d.label, spec, g[:3], want[:3], twin.get(id(d), g)[:3], third))
    if counts is not None:
        have = (ctx.b.fused_documents(ctx.h), ctx.b.redo_documents(ctx.h))
        assert have == counts, "%s: fused_documents, redo_documents = %r, expected %r" % (what, have, counts)
    return len(got)


# decoder settings (the ones tests/test_emu_parity.py::test_block_decoders_agree uses): the whole head staged, only the op / delete-start
# columns, nothing; two launches; the lane decoder
DECODER_SETTINGS = [("default", {}), ("lane", {"LM_DECODE": "0"}), ("unstaged", {"LM_DEC_SLOT": "16", "LM_DEC_SLOT_BIG": "0"}),
                    ("slot-64", {"LM_DEC_SLOT": "64", "LM_DEC_SLOT_BIG": "0"}), ("slot-160", {"LM_DEC_SLOT": "160", "LM_DEC_SLOT_BIG": "0"}),
                    ("slot-320", {"LM_DEC_SLOT": "320", "LM_DEC_SLOT_BIG": "0"}),
                    ("two-launches-64-320", {"LM_DEC_SLOT": "64", "LM_DEC_SLOT_BIG": "320", "LM_DEC_BIG_MODE": "2"}),
                    ("two-launches-160-4096", {"LM_DEC_SLOT": "160", "LM_DEC_SLOT_BIG": "4096", "LM_DEC_BIG_MODE": "2"}),
                    ("columns-launch-320", {"LM_DEC_SLOT": "320"})]


# --------------------------------------------------------------------------------------------- the other entry points: steps, snapshots
def chunked(reps):
    """every replica's own changes as blobs of one to four changes (tests/_resident.py), for delivery in steps"""
    return _resident.chunked_blobs(reps, random.Random(5))


def as_snapshot(reps):
    """ONE FastSnapshot of everything the replicas hold: the change blocks sit in its ChangeStore, the state section holds placeholder
    values, so a reader takes the history path"""
    m = wire.Replica((1 << 50) + 1)
    for r in reps:
        m.merge_from(r)
    return [m.export_snapshot()]


def path_docs():
    """the documents that go through the step and snapshot entry points: every third fuzz session, the documents of 7 / 8 / 9 blocks,
    the many-change blocks, the segment-boundary block"""
    return list(fuzz_docs()[0][::3]) + list(block_count_docs()) + [many_change_doc(n) for n in MANY] + [boundary_doc()]


def path_entries(suffix, write):
    out = []
    for i, d in enumerate(path_docs()):
        w = d.written(suffix, write)
        out += [(w, None), (w, ALL_SPECS[i % len(ALL_SPECS)]), (w, ALL_SPECS[(i + 7) % len(ALL_SPECS)])]
    return out


N_STEPS = 3


def run_steps(ctx, docs, specs, what=""):
    """`docs` as RESIDENT documents under `specs` (one form per document, None = canonical): the blobs of each in three steps
    (stage + import_more), every step rendered.  Every status 0, the last step's result the model's.
    -> (resident_fresh() after every step, the results of every step): the caller compares both with the canonical run's."""
    blobs = [d.blobs(spec) for d, spec in zip(docs, specs)]
    fresh, results = [], []
    for k in range(N_STEPS):
        now = [b[k::N_STEPS] for b in blobs]
        if k == 0:
            ctx.stage(now)
            ctx.import_more([[] for _ in now])
        else:
            ctx.import_more(now)
        ctx.run()
        got = ctx.fetch()
        fresh.append(ctx.resident_fresh())
        results.append(got)
        for d, spec, g in zip(docs, specs, got):
            assert g[0] == 0, (what, d.label, spec, k, g[:2])
            if k == N_STEPS - 1:
                assert g == d.expect(), "%s %s under %r:\n got   %r\n model %r" % (what, d.label, spec, g[:3], d.expect()[:3])
    return fresh, results


def check_steps(ctx, what=""):
    """the path documents in steps, canonical and under two forms each: the variants' results after EVERY step and their
    resident_fresh() are the canonical run's — every document is replayed from the empty version at the first step and none afterwards"""
    docs = [d.written(", in steps", chunked) for d in path_docs()]
    fresh, canon = run_steps(ctx, docs, [None] * len(docs), what)
    assert fresh == [len(docs), 0, 0], (what, fresh)
    for k in (0, 7):
        specs = [ALL_SPECS[(i + k) % len(ALL_SPECS)] for i in range(len(docs))]
        f, got = run_steps(ctx, docs, specs, what)
        assert f == fresh, (what, k, f, fresh)
        for step, (a, b) in enumerate(zip(got, canon)):
            for d, spec, x, y in zip(docs, specs, a, b):
                assert x == y, "%s %s under %r, step %d:\n got  %r\n twin %r" % (what, d.label, spec, step, x[:3], y[:3])
    return 3 * len(docs)


def check_message_sum(ctx):
    """the decoders sum the message-length column with rle_sum_uvar (the rest of a run at once) and only BOUND the sum by the message
    bytes, so no legal document depends on it: three changes with four-byte messages whose length column claims one run of 3 x 6 = 18
    bytes for the 12 that are there — LM_DATA_CORRUPTION (the reference maps every failure of the change_meta columns to it), on the
    device and in the oracle.  A sum that takes a run's value once (6 + 6 = 12) accepts the block."""
    r = wire.Replica(9)
    for i in range(3):
        r.map_set("m", "k", i); r.commit("abcd")
    d = Doc("message lengths that claim a run of 3 x 6 bytes for 12", [r], write=one_block_each)
    lie = d.blobs({"any_rle": {"msg_len": ("segments", lambda vals: [("run", len(vals), 6)])}})
    got = ctx.merge_batch([lie, d.blobs()])
    assert got[0][:2] == (3, b"") and got[1] == d.model.result(), [g[:2] for g in got]
    assert _oracle.merge(lie)[:2] == (3, b"")


def check_limits(ctx):
    """documents beyond the limits: the same STATUS under every form, no rendering — a position of 2^35 is LM_DECODE_ERROR (`prop` is an
    i32; the oracle says the same), a delete that names a counter near 2^31 is LM_DATA_CORRUPTION (the kernels compare a delete's
    targets with the elements at its position and refuse a mismatch, NEXT.md 0. item 6; the oracle applies it by position)"""
    for d, want in zip(beyond_limits_docs(), (1, 3, 3)):
        got = ctx.merge_batch([d.blobs(s) for s in (None, {"any_rle": "lit1"}, {"any_rle": "run1"}, {"any_rle": "mixed"}, {"any_rle": "split"})])
        assert all(g[:2] == (want, b"") for g in got), (d.label, [g[:2] for g in got])
    assert _oracle.merge(beyond_limits_docs()[0].blobs())[:2] == (1, b"")


def run_snapshots(ctx, entries, what=""):
    """snapshot entries as one batch: every status 0, a variant's whole result its canonical twin's, the twin's the oracle's on the
    same bytes, and the JSON of every key the model shows the model's (a snapshot also shows the roots of its state section)"""
    import json
    got = ctx.merge_batch([d.blobs(spec) for d, spec in entries])
    twin = {id(d): g for (d, spec), g in zip(entries, got) if spec is None}
    for (d, spec), g in zip(entries, got):
        assert g[0] == 0 and g == twin[id(d)], "%s %s under %r:\n got  %r\n twin %r" % (what, d.label, spec, g[:3], twin[id(d)][:3])
        if spec is None:
            assert g == _oracle.merge(d.blobs()), (what, d.label)
            shown, want = json.loads(g[1]), json.loads(d.model.json())
            assert all(shown[k] == v for k, v in want.items()) and g[2] == d.model.vv(), (what, d.label)
    return len(got)


# ------------------------------------------------------------------------------------------------------------- Map documents: the path
def map_path_docs():
    return [d for d in fuzz_docs()[0] if d.label.startswith("map")] + list(big_key_table_docs()) + [d for d in width_docs() if "Map rows" in d.label]


# (fused_documents, redo_documents) of the 17 documents of map_path_docs() as ONE batch, per setting of _merge_docs_map.SETTINGS, with
# LM_DEC_SLOT_BIG either way.  Literals, observed once on the kernel-logic harness and explained by the source: with k_map_fused on it
# takes all 17; it hands over (DF_REDO) the three blocks of 8,191 / 8,192 / 8,200 rows — more than MF_RMAX = 1,024 rows in a block — and
# under LM_HT_OPT=64 every document that holds more than 32 distinct (Map, key) pairs: all but one.
MAP_PATHS = {"fused": (17, 3), "LM_MAP_FUSED=0": (0, 0), "LM_LWW_LDS=0": (0, 0), "LM_HT_OPT=64": (17, 16), "LM_DECODE=0": (17, 3)}


def check_map_paths(ctx, name, oracle=None):
    """canonical, then three batches of variants: every result the model's, every batch's path counts the literal of its setting —
    a form must not move a document off (or onto) the fused path, and neither may a change move canonical and variant together"""
    docs = map_path_docs()
    assert len(docs) == 17
    run_entries(ctx, [(d, None) for d in docs], name, oracle, counts=MAP_PATHS[name])
    for k in (0, 4, 7):
        variants = [(d, ALL_SPECS[(i + k) % len(ALL_SPECS)]) for i, d in enumerate(docs)]
        run_entries(ctx, variants, name, oracle, counts=MAP_PATHS[name])
    return 4 * len(docs)
