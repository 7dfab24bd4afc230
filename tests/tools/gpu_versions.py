"""lm_versions on resident configs[1]-shaped documents (BASELINE.json: 100k-op trace, two concurrent peers): k_version's time for one
query of each op per document next to k_cursor (8 queries per document) on the same batch (lm_set_profiling(1)); the first lm_frontiers call (one
heads launch for all documents, wall time) beside them.  A record, not a test and not a target.
usage: python tests/tools/gpu_versions.py [docs] [base_ops] [branch_ops]     (one GPU step; run it under `timeout -k 10`)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loro_amd
from loro_amd import workload
from loro_amd._cabi import VER_TO_VV, VER_TO_FRONTIERS, VER_MINIMIZE, VER_CMP, VER_CMP_DOC

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
N_BASE = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
N_BRANCH = int(sys.argv[3]) if len(sys.argv) > 3 else 25000
TEXT = "cid:root-text:Text"

if __name__ == "__main__":
    import _versions_ref as R
    tpl = workload.Cfg2Template(N_BASE, N_BRANCH, seed=0, commit_every=10, fuse=True)
    docs = [tpl.stamp(d) for d in range(DOCS)]
    out = {"docs": DOCS, "ops_per_doc": N_BASE + 2 * N_BRANCH}
    with loro_amd.MergeEngine(0) as e:
        e.set_profiling(1)
        e.stage(docs); e.import_more([[] for _ in docs]); e.run()
        t = time.perf_counter()
        heads = [e.frontiers(d, 0) for d in range(DOCS)]
        out["lm_frontiers_all_documents_wall_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        assert all(h is not None for h in heads)
        ids = [R.decode((0, 0, h))[0] for h in heads]
        out["heads_of_document_0"] = len(ids[0])
        vvs = e.versions([(d, VER_TO_VV, heads[d]) for d in range(DOCS)])
        assert all(v[0] == 0 for v in vvs)
        qs = []
        for d in range(DOCS):
            older = R.enc_frontiers([(ids[d][0][0], 10)])
            qs += [(d, VER_TO_VV, heads[d]), (d, VER_TO_FRONTIERS, vvs[d][2]), (d, VER_MINIMIZE, R.enc_frontiers(ids[d] + [(ids[d][0][0], 10)])),
                   (d, VER_CMP, heads[d], older), (d, VER_CMP_DOC, heads[d])]
        best_wall, best_k = 1e9, 1e9
        for _ in range(3):
            e.run()                                       # (clears the stage list: the next call's k_version entry stands alone)
            t = time.perf_counter()
            got = e.versions(qs)
            wall = time.perf_counter() - t
            k = sum(ms for n, ms in e.kernel_times() if n == "k_version")
            best_wall, best_k = min(best_wall, wall), min(best_k, k)
        for d in range(DOCS):
            g = got[5 * d:5 * d + 5]
            assert g == [(0, 0, vvs[d][2]), (0, 0, heads[d]), (0, 0, heads[d]), (0, 1, b""), (0, 0, b"")], (d, g)
        out["five_ops_per_document"] = {"k_version_ms": round(best_k, 3), "lm_versions_wall_ms_incl_python": round(best_wall * 1e3, 1), "queries": len(qs)}
        cq = [(d, TEXT, (ids[d][0][0], c), 0) for d in range(DOCS) for c in range(0, 8000, 1000)]
        best_c = 1e9
        for _ in range(3):
            e.run()
            e.cursor_pos(cq)
            best_c = min(best_c, sum(ms for n, ms in e.kernel_times() if n == "k_cursor"))
        out["k_cursor_ms_8_queries_per_document"] = round(best_c, 3)
    print(json.dumps(out))
