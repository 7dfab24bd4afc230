"""The rendering sites of tests/_values.py, one function each: build the documents, run them as ONE batch through a context (the
kernel-logic harness or the HIP library), compare byte for byte with the plain Python expectation and with the oracle, and return
the counters that prove the intended path ran.  tests/test_values.py calls them in process on the harness with thinned corpora;
tests/test_gpu_zz_values.py runs each in a child process of its own (`python tests/_value_sites.py <site>`: the whole corpora on
the device, under a time limit)."""
import contextlib, json, os, sys, time

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _oracle
import _values as V


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(site, got, want, what="the Python expectation"):
    """got: [(status, json, …)] or [(status, bytes)]; want: [bytes] — equality of bytes, the first difference in the message"""
    assert len(got) == len(want), (site, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g[0] != 0 or g[1] != w:
            j = next((k for k in range(min(len(g[1]), len(w))) if g[1][k] != w[k]), min(len(g[1]), len(w)))
            lo = max(0, j - 48)
            raise AssertionError("%s: document %d differs from %s: status %d, byte %d of %d / %d\n  got  …%r\n  want …%r"
                                 % (site, i, what, g[0], j, len(g[1]), len(w), g[1][lo:j + 32], w[lo:j + 32]))


def _run(site, c, reps, want, docs=None):
    docs = V.docs_of(reps) if docs is None else docs
    got = c.merge_batch(docs)
    _same(site, got, want)
    ora = _oracle.merge_batch(docs, threads=8)
    _same(site + " (oracle)", ora, want)
    assert got == ora, site         # (version vectors and pending counts too)
    return docs, got


def _thin(xs, full, step):
    return xs if full else xs[::step]


def site_list(ctx, full):
    """1. List items — the whole f64 corpus; the documents overflow the optimistic slab, and are rendered once more with every
    document forced through the exact-size pass"""
    bits = V.f64_corpus() if full else V.f64_subset()[::4]
    reps, want = V.list_f64(bits)
    with ctx() as c:
        docs, got = _run("list items", c, reps, want)
        overflowed = c.sizing()[4]
        with _env(LM_SLAB_CAP="16"):
            _same("list items, exact-size pass", c.merge_batch(docs), want)
            forced = c.sizing()[4]
    assert overflowed > 0 and forced == len(docs), (overflowed, forced, len(docs))
    return {"documents": len(docs), "doubles": len(bits), "slab_overflow_documents": overflowed, "forced_exact_size_documents": forced}


def _map_sets(full):
    ints = V.i64_corpus()
    bits = _thin(V.f64_subset(), full, 8)
    kinds = [V.f64_generator(b) for b in bits]
    if full:
        assert len(bits) >= 5000 and kinds.count("u128") >= 2000 and kinds.count("big") >= 2000
    mixed, plain, items = V.map_mixed(bits, ints), V.map_plain(ints), V.list_ints(ints)
    for name, (_, want) in (("mixed", mixed), ("plain", plain), ("items", items)):     # each integer in all three sets
        blob = b"".join(want)
        for v in ints:
            assert (b":%d," % v in blob or b":%d}" % v in blob) if name != "items" else (b",%d," % v in blob or b"[%d," % v in blob or b",%d]" % v in blob), (name, v)
    return bits, mixed, plain, items


def site_map(ctx, full):
    """2. Map entry values: doubles among integers in 64-entry groups (entry by entry: sink_i64), the same integers in all-plain
    groups (the per-lane formatter) and as List items"""
    bits, mixed, plain, items = _map_sets(full)
    reps = mixed[0] + plain[0] + items[0]
    want = mixed[1] + plain[1] + items[1]
    with ctx() as c:
        docs, _ = _run("map entries", c, reps, want)
    return {"documents": len(docs), "doubles": len(bits), "integers": len(V.i64_corpus())}


def site_nested(ctx, full):
    """3. nested values: list in list, map values of <= 64 entries, of 65-70 entries, and an exhausted frame pool"""
    bits = V.f64_subset()[::2] if full else V.f64_subset()[::12]
    reps, want = V.nested(bits, V.i64_corpus(), V.str_corpus())
    with ctx() as c:
        docs, _ = _run("nested values", c, reps, want)
    return {"documents": len(docs), "doubles": len(bits)}


def site_movable(ctx, full):
    """4. MovableList insert and set"""
    bits = V.f64_subset()[1::2] if full else V.f64_subset()[1::12]
    reps, want = V.movable(bits, V.i64_corpus(), V.str_corpus())
    with ctx() as c:
        docs, _ = _run("movable list", c, reps, want)
    return {"documents": len(docs), "doubles": len(bits)}


def site_richtext(ctx, full):
    """5. rich-text attribute values (k_richtext) — against the Python expectation and the oracle's richtext values"""
    bits = V.f64_subset()[::3] if full else V.f64_subset()[::20]
    reps, want = V.richtext(bits, V.i64_corpus(), V.str_corpus())
    docs = V.docs_of(reps)
    with ctx() as c:
        res = c.merge_batch(docs)
        got = c.richtext()
    _same("richtext attribute values", got, want)
    ora = _oracle.richtext_batch(docs)
    _same("richtext attribute values (oracle)", ora, want)
    assert got == ora and res == _oracle.merge_batch(docs, threads=8)
    return {"documents": len(docs), "doubles": len(bits)}


def site_snapshot(ctx, full):
    """6. the snapshot state path: the values cross from the state section's postcard encoding to the op-value codec on the host"""
    import test_emu_snapshot as S
    c_ = V.f64_corpus()
    sub = V.f64_subset()
    ints, strs = V.i64_corpus(), V.str_corpus()
    parts = [V.list_f64(c_[-20000::5] + c_[:20000:20] if full else c_[-20000::80] + sub[::40]),      # (the tail of the corpus: uniform random bit patterns)
             V.map_mixed(_thin(sub, full, 10)[::4], ints), V.map_plain(ints), V.list_ints(ints),
             V.nested(_thin(sub, full, 8)[::8], ints, strs), V.strings(strs)]
    reps = [r for p in parts for r in p[0]]
    want = [w for p in parts for w in p[1]]
    docs = [[S.real_snapshot(r)] for r in reps]
    with ctx() as c:
        _run("snapshot state path", c, reps, want, docs=docs)
        n_state = c.b.state_documents(c.h)
    assert n_state == len(docs), (n_state, len(docs))
    return {"documents": len(docs), "state_documents": n_state}


def site_fused(ctx, full):
    """7. the folded Map path (lm_k_map_fused.h), then the same documents through the row tables"""
    bits, mixed, plain, _ = _map_sets(full)
    keys = V.map_strings(V.str_corpus())
    reps, want = mixed[0] + plain[0] + keys[0], mixed[1] + plain[1] + keys[1]
    with ctx() as c, _env(LM_MF_MIN_ROWS="1", LM_MF_CHG_RATIO="0"):
        docs, got = _run("folded map path", c, reps, want)
        n_fused, n_redo = c.b.fused_documents(c.h), c.b.redo_documents(c.h)
        with _env(LM_MAP_FUSED="0"):
            rows = c.merge_batch(docs)
            n_rows = c.b.fused_documents(c.h)
    assert n_fused == len(docs) and n_rows == 0, (n_fused, n_rows, len(docs))
    assert rows == got
    return {"documents": len(docs), "doubles": len(bits), "fused_documents": n_fused, "redo_documents": n_redo}


def site_strings(ctx, full):
    """8. strings as Map values, List items, Map keys and Text content"""
    reps, want = V.strings(V.str_corpus())
    with ctx() as c:
        docs, _ = _run("strings", c, reps, want)
    return {"documents": len(docs), "strings": len(V.str_corpus())}


SITES = {"list": site_list, "map": site_map, "nested": site_nested, "movable": site_movable, "richtext": site_richtext,
         "snapshot": site_snapshot, "fused": site_fused, "strings": site_strings}


if __name__ == "__main__":
    import loro_amd
    t0 = time.time()
    out = SITES[sys.argv[1]](lambda: loro_amd.MergeEngine(0), True)
    out["site"], out["seconds"] = sys.argv[1], round(time.time() - t0, 2)
    print(json.dumps(out))
