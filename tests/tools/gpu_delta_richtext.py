"""lm_delta_richtext on configs[1]-shaped RESIDENT documents that carry marks (base by peer A; A and B continue concurrently with the
same actions; ≈1 % of the actions are marks of a few keys and values, unmarks among them): the base is staged and run, the two
branches are imported and run, then one query per document asks for the delta from the end of the base to the latest version.
Reports k_rtdelta_mark + k_rtdelta next to k_delta_mark + k_delta on the same documents and queries in the same process, the emit
stage of the same run, the wall time of lm_richtext, and the bytes the call copies back (lm_delta_bytes) against the bytes of
lm_richtext for the same documents — the parent's only way to tell a subscriber about styles.
Parity of the timed call, for every distinct document: its ops applied to lm_richtext's spans at the end of the base give
lm_richtext's spans at the latest version, and without their attributes they are lm_delta's ops.
Not a test.  usage: python tests/tools/gpu_delta_richtext.py [docs] [base_ops] [branch_ops]   (one GPU step; run it under `timeout -k 10`)"""
import json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loro_amd
from loro_amd import wire, workload

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 512
N_BASE = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
N_BRANCH = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
DISTINCT = 4
CID = wire.root_cid("text", wire.KIND_TEXT)


def write(r, acts, rng, upper=False, commit_every=10):
    ids = r.seq.setdefault(CID, [])
    for k, (pos, dl, ch) in enumerate(acts):
        if len(ids) >= 2 and rng.random() < 0.01:
            s = rng.randrange(len(ids) - 1)
            r.text_mark("text", s, rng.randrange(s + 1, min(len(ids), s + 40)), rng.choice(["bold", "link", "color"]), rng.choice([True, True, None, "https://x.y/", 7, "red"]))
        elif dl:
            r.text_delete("text", min(pos, len(ids) - 1), 1)
        else:
            r.text_insert("text", min(pos, len(ids)), ch.upper() if upper else ch)
        if (k + 1) % commit_every == 0:
            r.commit()
    r.commit()


def gen(d):
    acts = workload.synthetic_trace(N_BASE + N_BRANCH, seed=d)
    a, b = wire.Replica(2 * d + 1), wire.Replica(2 * d + 2)
    write(a, acts[:N_BASE], random.Random(d))
    base_vv = dict(a.vv)
    b.merge_from(a)
    b.seq = {k: list(v) for k, v in a.seq.items()}
    write(a, acts[N_BASE:], random.Random(1000 + d))
    write(b, acts[N_BASE:], random.Random(2000 + d), upper=True)
    return [export_to(a, base_vv), a.export(from_vv=base_vv), b.export(from_vv=base_vv)]


def export_to(r, vv):
    own = wire.Replica(r.peer)
    own.changes = {r.peer: [c for c in r.changes[r.peer] if c.ctr_end <= vv[r.peer]]}
    return own.export()


def pairs(rich):
    return [(c, s.get("attributes", {})) for spans in [json.loads(rich).get("cid:root-text:Text", [])] for s in spans for c in s["insert"]]


if __name__ == "__main__":
    import _delta_richtext
    base = [gen(d) for d in range(DISTINCT)]
    docs = [[bytes(bytearray(b)) for b in base[i % DISTINCT]] for i in range(DOCS)]
    print("generated", DOCS, "documents", flush=True)
    out = {"docs": DOCS, "ops_per_doc": N_BASE + 2 * N_BRANCH}
    with loro_amd.MergeEngine(0) as e:
        e.set_profiling(1)
        e.stage([d[:1] for d in docs]); e.run()
        vv1 = [r[2] for r in e.fetch()]
        rich1 = e.richtext()
        e.import_more([d[1:] for d in docs]); e.run()
        out["k_emit_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_emit")), 3)
        res = e.fetch()
        ts = []
        for _ in range(3):
            t = time.perf_counter(); rich2 = e.richtext(); ts.append(time.perf_counter() - t)
        out["lm_richtext_wall_ms"] = round(min(ts) * 1e3, 1)
        out["json_bytes"] = sum(len(r[1]) for r in res)
        out["richtext_bytes"] = sum(len(r[1]) for r in rich2)
        q = [(d, vv1[d]) for d in range(DOCS)]

        def timed(call, names):
            best = None
            for _ in range(3):
                n0 = len(e.kernel_times())
                t = time.perf_counter()
                got = call()
                wall = time.perf_counter() - t
                k = {}
                for n, ms in e.kernel_times()[n0:]:           # (a call that took the overflow path lists its kernel twice: summed)
                    k[n] = k.get(n, 0.0) + ms
                if best is None or sum(k.values()) < sum(best[1].values()):
                    best = (got, k, wall, int(e.b.delta_bytes(e.h)))
            return best
        plain, kp, wp, bp = timed(lambda: e.delta(q, 0), None)
        got, kr, wr, br = timed(lambda: e.delta_richtext(q, 0), None)
        for d in range(DISTINCT):
            assert got[d][0] == 0 and plain[d][0] == 0, (got[d][:2], plain[d][:2])
            ops = json.loads(got[d][2]).get("cid:root-text:Text", [])
            after, target = _delta_richtext.apply_ops(pairs(rich1[d][1]), ops, 0, d), pairs(rich2[d][1])
            assert after == target, "document %d: the delta applied to lm_richtext at A is not lm_richtext at V" % d
            assert _delta_richtext.strip(ops) == json.loads(plain[d][2]).get("cid:root-text:Text", []), "document %d: not lm_delta's ops" % d
        assert all(g == got[i % DISTINCT] for i, g in enumerate(got)), "instances differ"
        for name, k in (("delta", kp), ("rtdelta", kr)):
            for n, ms in k.items():
                out[("rt_" if name == "rtdelta" and n == "k_delta_pack" else "") + n + "_ms"] = round(ms, 3)
        out["lm_delta_wall_ms"], out["lm_delta_richtext_wall_ms"] = round(wp * 1e3, 1), round(wr * 1e3, 1)
        out["delta_d2h_bytes"], out["delta_richtext_d2h_bytes"] = bp, br
        out["delta_richtext_json_bytes"] = sum(len(g[2]) for g in got)
        out["attributed_ops_doc0"] = got[0][2].count(b'"attributes"')
        out["other_changed_bits"] = sorted({g[1] for g in got})
        assert e.fetch() == res
    print(json.dumps(out))
