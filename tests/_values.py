"""Scalar rendering at its edges: corpora of f64 bit patterns, integers and strings, PLAIN references of their JSON text
(no kernel or oracle code: `repr(float)` + ryu's layout rules, `str(int)`, `json.dumps`), and document builders that put the
values at every site the renderer writes them from (lm_k_emit.h sink_value / sink_i64 / the 64-entries-per-step Map groups /
sink_escaped / cp_bytes, lm_f64.h).  Shared by tests/test_values.py (kernel-logic harness) and tests/test_gpu_zz_values.py."""
import json, math, random, struct

from loro_amd import wire

MAX_F64_PER_DOC = 128     # one wave renders a document serially; the 40-limb branch of f64_json is the slowest thing it can meet
_M52 = (1 << 52) - 1
_SIGN = 1 << 63


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


# ---------------------------------------------------------------------------------------------------------------- references
def ryu_layout(x):
    """JSON text of a double as serde_json / ryu's pretty printer lays it out, from Python's shortest round-trip digits."""
    if x != x or x in (math.inf, -math.inf):
        return "null"
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    if x == 0:
        return sign + "0.0"
    mant, _, ex = repr(abs(x)).partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    k = len(ip) + (int(ex) if ex else 0) - (len(ip + fp) - len(digits))    # value = 0.d1d2…dn × 10^k
    digits = digits.rstrip("0")
    nd = len(digits)
    if nd <= k <= 16:
        body = digits + "0" * (k - nd) + ".0"
    elif 0 < k <= 16:
        body = digits[:k] + "." + digits[k:]
    elif -5 < k <= 0:
        body = "0." + "0" * (-k) + digits
    else:
        body = digits[0] + ("." + digits[1:] if nd > 1 else "") + "e" + str(k - 1)
    return sign + body


def to_json(v):
    """canonical JSON text of a plain value: map keys in bytewise order, no spaces"""
    if v is None:
        return "null"
    if v is True:
        return "true"
    if v is False:
        return "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        return ryu_layout(v)
    if isinstance(v, str):
        return json.dumps(v, ensure_ascii=False)
    if isinstance(v, (bytes, bytearray)):
        return "[" + ",".join(str(b) for b in v) + "]"
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(to_json(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ",".join(to_json(k) + ":" + to_json(v[k]) for k in sorted(v, key=lambda s: s.encode("utf-8"))) + "}"
    raise TypeError(type(v))


def doc_json(roots):
    """expected bytes of a document whose root containers hold `roots` (name -> plain value; a Text root is its string)"""
    return to_json(roots).encode("utf-8")


def f64_generator(bits):
    """which part of f64_json (lm_f64.h) a bit pattern is rendered by: 'null' | 'zero' | 'int' (the <n>.0 path) | 'u128' (the
    two-register digit generator, -121 <= e2 <= 60) | 'big' (the limb generator).  Bookkeeping of the tests, not a reference."""
    be, frac = (bits >> 52) & 0x7FF, bits & _M52
    if be == 0x7FF:
        return "null"
    if be == 0 and frac == 0:
        return "zero"
    f = (frac | (1 << 52)) if be else frac
    e2 = be - 1075 if be else -1074
    if -53 < e2 <= 0 and f & ((1 << -e2) - 1) == 0 and (f >> -e2) < 10 ** 16:
        return "int"
    return "u128" if -121 <= e2 <= 60 else "big"


def f64_scale(bits):
    """e2 + bitlen - 1, the integer the decimal-exponent estimate of f64_json is computed from (-1074..1023)"""
    be, frac = (bits >> 52) & 0x7FF, bits & _M52
    f = (frac | (1 << 52)) if be else frac
    return (be - 1075 if be else -1074) + f.bit_length() - 1


# ------------------------------------------------------------------------------------------------------------------ corpora
_F64 = None


def f64_corpus():
    """deterministic list of f64 bit patterns (no duplicates)"""
    global _F64
    if _F64 is not None:
        return _F64
    rng = random.Random(0xF64)
    out = []
    for be in range(0, 2047):                      # every biased exponent: both ends and the middle of its binade
        out += [(be << 52) | fr for fr in (0, 1, _M52, 1 << 51, rng.getrandbits(52))]
        if be:
            out.append((be << 52) - 1)             # the predecessor of fraction 0 (the uneven gap below a power of two)
    for s in range(0, 52):                         # every denormal bit length 1..52
        out += [1 << s, (2 << s) - 1] + ([3 << (s - 1)] if s else [])
    for k in range(-323, 309):                     # powers of ten and their neighbours
        b = bits_of(float("1e%d" % k))
        out += [b - 1, b, b + 1]
    for nd in range(1, 18):                        # decimals of every digit count over the whole range of decimal exponents:
        for ex in range(-323, 309):                # four per exponent where the two-register generator works, every other exponent elsewhere
            for _ in range(4 if -21 <= ex <= 34 else (ex + nd) & 1):
                m = rng.randint(10 ** (nd - 1), 10 ** nd - 1)
                x = float("%de%d" % (m, ex - nd + 1))
                if x != 0 and x != math.inf:
                    out.append(bits_of(x))
    for _ in range(1400):                          # everyday values
        out += [bits_of(rng.uniform(-1e3, 1e3)), bits_of(rng.random() * 10.0 ** rng.randint(-8, 20)), bits_of(round(rng.uniform(-1e4, 1e4), rng.randint(0, 6)))]
    for x in (1e15, 1e16, 1e17, 1e-5, 1e-6, 1e-7, 1e21, 1e22, 123456789012345680.0, 0.1, 0.3, 2 / 3, 5e-324, 1.7976931348623157e308, 2.2250738585072014e-308,
              2.225073858507201e-308, 9007199254740991.0, 9007199254740992.0, 9007199254740994.0, 9999999999999998.0, 9999999999999996.0, 1e16 + 2, 0.5, 1.5,
              -2.5e-7, 3.0e22, 0.0001, 0.00001, 0.000011, 0.00009999999999999999, 1234567890123456.0, 1234567890123456.8, 12345678901234567.0):
        b = bits_of(x)
        out += [b, b + 1] + ([b - 1] if b else [])
    for nd in range(1, 17):                        # integer-valued doubles that take the <n>.0 path, every digit count
        out += [bits_of(float(v)) for v in (10 ** (nd - 1), 10 ** nd - 1, 10 ** (nd - 1) + 1, rng.randint(10 ** (nd - 1), 10 ** nd - 1), rng.randint(10 ** (nd - 1), 10 ** nd - 1))
                if v < 2 ** 53]
        out.append(bits_of(float(rng.randint(1, 9) * 10 ** (nd - 1))))
    for j in range(-20, 70):                       # 10^23 · 2^j lies exactly half way between two doubles (5^23 takes 54 bits) and is a short
        b = bits_of(float(10 ** 23 * 2 ** j) if j >= 0 else float(10 ** 23) / 2 ** -j)   # decimal: the lower neighbour's mantissa is even, so the
        out += [b - 1, b, b + 1]                   # interval's end belongs to it and these few digits are its shortest form — in both generators
    for e2 in list(range(-123, -118)) + list(range(58, 63)):   # where the two digit generators hand over
        be = e2 + 1075
        out += [(be << 52) | fr for fr in (0, 1, 2, _M52, _M52 - 1, 1 << 51, (1 << 51) - 1)] + [(be << 52) | rng.getrandbits(52) for _ in range(24)]
    out += [0, _SIGN, 0x7FF << 52, (0x7FF << 52) | _SIGN, 0x7FF8 << 48, (0x7FF << 52) | 1, 0xFFF8 << 48, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
            0x7FF4 << 48, (0x7FF8 << 48) | 0xDEADBEEF]
    out += [b | _SIGN for b in out[::5]]           # a negated copy of a subset
    out += [rng.getrandbits(63) for _ in range(20000)]
    _F64 = list(dict.fromkeys(out))
    return _F64


def f64_subset(n_each=2600):
    """a spread of the corpus with at least `n_each` values of each digit generator, and every value of the other kinds"""
    c = f64_corpus()
    by = {}
    for b in c:
        by.setdefault(f64_generator(b), []).append(b)
    out = []
    for kind in ("u128", "big"):
        xs = by[kind]
        step = max(1, len(xs) // n_each)
        out += xs[::step]
    out += by["int"][::4] + by["zero"] + by["null"][:12]
    return out


def i64_corpus():
    out = []
    for k in range(19):
        p = 10 ** k
        out += [p, -p, p - 1, -(p - 1), p + 1, -(p + 1)]
    # a zero middle or low 9-digit chunk, chunks that need their leading zeros
    out += [k * 10 ** 9 for k in (2, 7, 999999999, 1000000001, 123456789, -5, -999999999)]
    out += [k * 10 ** 18 for k in (2, 5, 9, -3, -9)]
    out += [10 ** 18 + 10 ** 9, 10 ** 18 + 1, 10 ** 18 + 10 ** 9 + 1, 9 * 10 ** 18 + 5, 5 * 10 ** 18 + 3 * 10 ** 9, 10 ** 18 + 999999999, 999999999999999999,
            1000000001000000001, 1000000000000000010, 1000000010, 1000000000000000100, -1000000001000000001, 9000000000000000000, 9223372036000000000,
            123456789012345678, 100000000200000000, 42, 2 ** 63 - 1, -(2 ** 63), 2 ** 63 - 2, -(2 ** 63) + 1, 2 ** 32, 2 ** 32 - 1, -(2 ** 32), 2 ** 31, -(2 ** 31) - 1]
    # every LEB128 width (the list of map_render_docs())
    out += [0, 1, -1, 63, 64, -64, -65, 8191, 8192, -8192, -8193, 2 ** 20, -(2 ** 20) - 1, 2 ** 27 - 1, 2 ** 27, 2 ** 34, -(2 ** 34) - 1, 2 ** 41, 2 ** 48,
            -(2 ** 48) - 1, 2 ** 55, 2 ** 62, -(2 ** 62)]
    return list(dict.fromkeys(out))


def str_corpus():
    out = [""]
    for b in range(0x80):
        out += [chr(b), "a" + chr(b) + "z"]
    out += ["é", "中", "😀", "aé中😀λz", "\u0080߿ࠀ￿\U00010000\U0010ffff", "ключ", "q\"uo\\te\n\t\x01é"]
    out.append("".join(chr(b) for b in range(0x20)))           # every control byte side by side: 2- and 6-byte escapes alternate
    out.append("\x01" * 64 + "\x1f" * 3)                        # 64 lanes of six bytes each
    out.append("k" * 24); out.append("k" * 25); out.append("é" * 12); out.append("é" * 12 + "x")   # 24 / 25 bytes: the plain-group key rule
    pat = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_"
    for n in (1, 63, 64, 65, 127, 128, 129, 200):
        s = (pat * 4)[:n]
        out.append(s)
        if n > 1:
            out.append(s[:-1] + "\"")                            # an escape in the last byte
            out.append("\\" + s[1:])
            out.append(("é" + s)[:n])                            # n scalars, n + 1 bytes
            out.append(("😀\n中" * n)[:n])
    for off in (62, 63, 64, 65):                                # a 6-byte escape (and a 2-byte one) astride the 64-lane chunk border
        for c in ("\x01", "\x7f", "\n", "\"", "\x1f\x00\x1e"):
            out.append("x" * off + c + "y" * 70)
            out.append("é" * (off // 2) + "z" * (off % 2) + c + "tail")
    return list(dict.fromkeys(out))


# ------------------------------------------------------------------------------------------------------------------ builders
# Every builder returns (replicas, expected JSON bytes per document); a document is [replica.export()] (docs_of) or, for the
# snapshot state path, [real_snapshot(replica)].
_PEER = [5000]


def _rep():
    _PEER[0] += 1
    return wire.Replica(_PEER[0])


def docs_of(reps):
    return [[r.export()] for r in reps]


def _chunks(xs, n):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


def list_f64(bits_list, per_doc=MAX_F64_PER_DOC):
    """site 1: doubles as List items"""
    reps, want = [], []
    for chunk in _chunks(bits_list, per_doc):
        vals = [f64_of(b) for b in chunk]
        r = _rep(); r.list_insert("l", 0, vals); r.commit()
        reps.append(r); want.append(doc_json({"l": vals}))
    return reps, want


def map_mixed(bits_list, ints, per_group=16, groups=8):
    """site 2, first set: Map entries in key order, every 64-entry group holds `per_group` doubles (the group is rendered entry by
    entry: the integers beside them go through sink_i64) — at most per_group * groups = 128 doubles per document"""
    assert per_group * groups <= MAX_F64_PER_DOC and 64 % per_group == 0
    stride = 64 // per_group
    reps, want = [], []
    at = 0
    for chunk in _chunks(bits_list, per_group * groups):
        r, m, fi = _rep(), {}, 0
        n_entries = max(64 * groups, len(ints) * 2)
        for i in range(n_entries):
            if i % stride == stride // 2 and fi < len(chunk) and i < 64 * groups:
                v = f64_of(chunk[fi]); fi += 1
            else:
                v = ints[at % len(ints)]; at += 1
            m["k%04d" % i] = v
            r.map_set("m", "k%04d" % i, v)
            if i % 100 == 99:
                r.commit()
        r.commit()
        assert fi == len(chunk)
        reps.append(r); want.append(doc_json({"m": m}))
    return reps, want


def map_plain(ints):
    """site 2, second set: only integers / bools / null under short keys — every group takes the 64-entries-per-step formatter"""
    reps, want = [], []
    for shift in (0, 17, 40):                      # each integer in several lanes
        r, m = _rep(), {}
        vals = ints[shift:] + ints[:shift] + [None, True, False]
        for i, v in enumerate(vals):
            k = "k%03d" % i if i % 5 else "key-of-24-bytes-----%04d" % i
            m[k] = v; r.map_set("m", k, v)
        r.commit()
        # the rule of the 64-entries-per-step formatter (lm_k_emit.h): were one entry not plain, its group would quietly go entry by entry
        assert all(len(k.encode()) <= 24 and not any(c < " " or c in '"\\' for c in k) for k in m)
        assert all(v is None or isinstance(v, (bool, int)) for v in m.values()) and {len(k.encode()) for k in m} >= {4, 24}
        reps.append(r); want.append(doc_json({"m": m}))
    return reps, want


def list_ints(ints):
    """site 2, third set: the integers as List items"""
    r = _rep(); r.list_insert("l", 0, list(ints)); r.commit()
    r2 = _rep(); r2.list_insert("l", 0, [[v] for v in ints] + [bytes(range(256))]); r2.commit()
    return [r, r2], [doc_json({"l": list(ints)}), doc_json({"l": [[v] for v in ints] + [bytes(range(256))]})]


def pool_fallbacks(v, top=0):
    """how many maps of <= 64 entries inside the plain value `v` the renderer cannot order in its pool (lm_k_emit.h sink_value:
    a map frame of n <= 64 entries takes n of the 256 slots while it is open, if they are free; otherwise, like a larger map,
    it is re-scanned for the next key each time).  Bookkeeping of the builders, not a reference."""
    if isinstance(v, dict):
        n = len(v)
        fits = n <= 64 and top + n <= 256
        return (1 if n <= 64 and not fits else 0) + sum(pool_fallbacks(x, top + n if fits else top) for x in v.values())
    if isinstance(v, (list, tuple)):
        return sum(pool_fallbacks(x, top) for x in v)
    return 0


def nested(bits_list, ints, strs):
    """site 3: the values inside a list inside a list, inside map values of <= 64 entries (ordered once), of 65-70 entries (the
    re-scan fallback) and under enough OPEN map frames of one value to exhaust the 256-slot pool: maps of 64 (63) entries nested
    in one another four deep hold all (all but four) slots, and the small maps of doubles, integers and strings inside them are
    rendered by the re-scan fallback although they have fewer than 64 entries — pool_fallbacks() counts them by the renderer's
    rule, and one 4-entry map fits the last four slots exactly"""
    reps, want = [], []
    pool = [f64_of(b) for b in bits_list]
    ii, si = 0, 0

    def others(n):
        nonlocal ii, si
        out = []
        for j in range(n):
            if j % 3 == 2:
                out.append(strs[si % len(strs)]); si += 1
            else:
                out.append(ints[ii % len(ints)]); ii += 1
        return out

    for di, chunk in enumerate(_chunks(pool, 120)):
        a, b, c, e = chunk[:30], chunk[30:60], chunk[60:90], chunk[90:]
        deep = [[a + others(20), [others(5), [a[:3]]]], "between"]
        m64 = {"f%02d" % (i * 37 % 64): v for i, v in enumerate(b + others(64 - len(b)))}
        n70 = 65 + di % 6
        m70 = {"g%02d" % (i * 41 % n70): v for i, v in enumerate(c + others(n70 - len(c)))}
        e = e + others(28 - len(e)) if len(e) < 28 else e

        def chain(width, inner, lv=0):     # `width`-entry maps four deep; one entry of each holds the next level, the others scalars
            m = {"e%02d" % (i * 29 % width): v for i, v in enumerate(others(width))}
            m["e%02d" % ((lv * 13 + 7 + di) % width)] = inner if lv == 3 else chain(width, inner, lv + 1)
            return m
        in_a = {"a%02d" % (i * 7 % 40): v for i, v in enumerate(e[:20] + others(20))}                   # 256 slots taken: re-scan
        in_c = {"c%d" % i: v for i, v in enumerate(e[20:25])}                                           # 252 taken, 5 entries: re-scan
        in_b = {"b2": e[25], "b0": {"z": e[26], "y": e[27], "x": others(3)}, "b3": others(2), "b1": None}   # 252 + 4: ordered; the map inside: re-scan
        frames = [chain(64, in_a), chain(63, in_c), chain(63, in_b), {"after": e[:2]}]
        assert pool_fallbacks(frames) == 3 and pool_fallbacks([deep, m64, m70]) == 0
        r = _rep()
        r.list_insert("l", 0, [deep, m64, m70])
        r.map_set("m", "sorted", m64); r.map_set("m", "rescan", m70); r.map_set("m", "pool", frames); r.map_set("m", "deep", deep)
        r.commit()
        reps.append(r)
        want.append(doc_json({"l": [deep, m64, m70], "m": {"sorted": m64, "rescan": m70, "pool": frames, "deep": deep}}))
    return reps, want


def movable(bits_list, ints, strs):
    """site 4: MovableList insert and set"""
    reps, want = [], []
    for di, chunk in enumerate(_chunks([f64_of(b) for b in bits_list], 120)):
        half = len(chunk) // 2
        ins = chunk[:half] + ints[di::7][:20] + strs[di::11][:10]
        sets = chunk[half:]
        r = _rep()
        r.mlist_insert("ml", 0, [0] * len(sets) + ins)
        r.commit()
        for i, v in enumerate(sets):
            r.mlist_set("ml", i, v)
        r.mlist_set("ml", len(sets), {"k": chunk[0], "j": [chunk[-1], ints[di % len(ints)]]})
        r.commit()
        final = list(sets) + [{"k": chunk[0], "j": [chunk[-1], ints[di % len(ints)]]}] + ins[1:]
        reps.append(r); want.append(doc_json({"ml": final}))
    return reps, want


def richtext(bits_list, ints, strs):
    """site 5: rich-text attribute values.  One Text per document, "a-b-c-…": letter i is marked with key "k" and value i, the
    dashes between them stay unmarked, so every value is a span of its own whatever the rule for merging equal neighbours says
    about NaNs and signed zeros.  (Marks are laid from the last letter to the first: the anchors of one mark never move the
    positions of the next.)  Returns (replicas, expected richtext bytes):
    {"cid:root-t:Text":[{"attributes":{"k":<value>},"insert":"a"},{"insert":"-"},…]} (canonical: keys in bytewise order)"""
    vals_all = [f64_of(b) for b in bits_list]
    reps, want = [], []
    for di, chunk in enumerate(_chunks(vals_all, 40)):
        vals = list(chunk) + [ints[(di * 3 + j) % len(ints)] for j in range(3)] + [strs[(di * 2 + j) % len(strs)] for j in range(2)]
        vals += [{"b": chunk[0], "a": [5e-324, 1.7976931348623157e308, ints[di % len(ints)]], "": strs[di % len(strs)]}, [chunk[-1], {"x": 5e-324}, None, True], None, True, False]
        text = "".join(chr(0x61 + i % 26) + "-" for i in range(len(vals)))
        r = _rep()
        r.text_insert("t", 0, text)
        for i in range(len(vals) - 1, -1, -1):
            r.text_mark("t", 2 * i, 2 * i + 1, "k", vals[i])
        r.commit()
        spans = []                                   # [attributes or None, text]; a mark with value null is an unmark: no attribute
        for i, v in enumerate(vals):
            for attr, ch in ((None if v is None else '{"k":%s}' % to_json(v), text[2 * i]), (None, "-")):
                if spans and attr is None and spans[-1][0] is None:
                    spans[-1][1] += ch
                else:
                    spans.append([attr, ch])
        body = ",".join(('{"attributes":%s,"insert":%s}' % (a, to_json(t))) if a else ('{"insert":%s}' % to_json(t)) for a, t in spans)
        reps.append(r)
        want.append(('{"cid:root-t:Text":[' + body + "]}").encode("utf-8"))
    return reps, want


def strings(strs):
    """site 8: the strings as Map values, List items, Map keys and Text content"""
    reps, want = [], []
    for chunk in _chunks(strs, 100):
        r = _rep()
        r.list_insert("l", 0, list(chunk))
        vm, km = {}, {}
        for i, s in enumerate(chunk):
            vm["v%03d" % i] = s; r.map_set("vals", "v%03d" % i, s)
            km[s] = i if i % 9 else s; r.map_set("keys", s, km[s])
        r.commit()
        reps.append(r); want.append(doc_json({"l": list(chunk), "vals": vm, "keys": km}))
    # Text content (cp_bytes): the strings end to end, sixty per Text container
    for chunk in _chunks(strs, 60):
        r = _rep()
        whole = ""
        for s in chunk:
            if s:
                r.text_insert("t", len(whole), s); whole += s
        r.commit()
        reps.append(r); want.append(doc_json({"t": whole}))
    # a nested map value whose keys are the strings (sink_string on the sorted frame and on the re-scan fallback)
    for chunk in _chunks(strs, 68):
        r = _rep()
        v = {s: [s] for s in chunk}
        r.list_insert("l", 0, [v, {s: 1 for s in chunk[:40]}]); r.commit()
        reps.append(r); want.append(doc_json({"l": [v, {s: 1 for s in chunk[:40]}]}))
    return reps, want


def map_strings(strs):
    """Map-only documents (what the folded Map path takes): the strings as values and as keys, integers and doubles beside them"""
    reps, want = [], []
    for chunk in _chunks(strs, 120):
        r, vm, km = _rep(), {}, {}
        for i, s in enumerate(chunk):
            vm["v%03d" % i] = s; r.map_set("vals", "v%03d" % i, s)
            km[s] = [i, 0.1 * i, -i][i % 3]; r.map_set("keys", s, km[s])
            if i % 25 == 24:
                r.commit()
        r.commit()
        reps.append(r); want.append(doc_json({"vals": vm, "keys": km}))
    return reps, want
