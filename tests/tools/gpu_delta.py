"""lm_delta on configs[1]-shaped RESIDENT documents (BASELINE.json: 100k-op trace, two concurrent peers): the base is staged and run,
the two branches are imported and run, then one query per document asks for the delta from the end of the base to the latest
version.  Reports k_delta_mark + k_delta next to the same run's emit stage (lm_set_profiling(1)) and the bytes lm_delta copies back (lm_delta_bytes) against the
JSON bytes lm_fetch would move — the parent's only way to serve a subscriber is emit + D2H of the full JSON.
Not a test.  usage: python tests/tools/gpu_delta.py [docs] [base_ops] [branch_ops]     (one GPU step; run it under `timeout -k 10`)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loro_amd
from loro_amd import workload

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
N_BASE = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
N_BRANCH = int(sys.argv[3]) if len(sys.argv) > 3 else 25000

if __name__ == "__main__":
    import _delta
    tpl = workload.Cfg2Template(N_BASE, N_BRANCH, seed=0, commit_every=10, fuse=True)
    docs = [tpl.stamp(d) for d in range(DOCS)]
    a, v = _delta.At(docs[0][:1]), _delta.At(docs[0])                        # document 0's answer: the parity check of the timed call
    want = {u: _delta.expected(a, v, u)[0] for u in (0, 1)}
    print("generated", DOCS, "documents; document 0's delta:", len(want[0]), "bytes", flush=True)
    out = {"docs": DOCS, "ops_per_doc": N_BASE + 2 * N_BRANCH}
    with loro_amd.MergeEngine(0) as e:
        e.set_profiling(1)
        e.stage([d[:1] for d in docs]); e.run()
        vv1 = [r[2] for r in e.fetch()]
        assert vv1[0] == a.vv
        e.import_more([d[1:] for d in docs]); e.run()
        out["lm_run_stage_ms"] = {n: round(ms, 3) for n, ms in e.kernel_times()}
        out["k_emit_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_emit")), 3)
        res = e.fetch()
        out["json_bytes"] = sum(len(r[1]) for r in res)
        q = [(d, vv1[d]) for d in range(DOCS)]
        best = None
        for units in (0, 1, 0):
            n0 = len(e.kernel_times())                    # (the stage list grows with every call: this call's entries are its tail)
            t = time.perf_counter()
            got = e.delta(q, units)
            wall = time.perf_counter() - t
            k = {}
            for n, ms in e.kernel_times()[n0:]:           # (a call that took the overflow path lists k_delta twice: summed)
                k[n] = k.get(n, 0.0) + ms
            assert got[0] == (0, 0, want[units]), "document 0 differs from the reference"
            assert all(g[0] == 0 and len(g[2]) == len(want[units]) for g in got), "stamped documents differ"
            if best is None or sum(k.values()) < sum(best["k"].values()):
                best = {"k": k, "wall": wall}
            out["delta_json_bytes"] = sum(len(g[2]) for g in got)
            out["delta_d2h_bytes"] = int(e.b.delta_bytes(e.h))   # what the call copied back: result rows + the packed answers
        out["k_delta_mark_ms"] = round(best["k"].get("k_delta_mark", 0.0), 3)
        out["k_delta_ms"] = round(best["k"].get("k_delta", 0.0), 3)
        out["k_delta_pack_ms"] = round(best["k"].get("k_delta_pack", 0.0), 3)
        out["lm_delta_wall_ms"] = round(best["wall"] * 1e3, 1)
        assert e.fetch() == res
    print(json.dumps(out))
