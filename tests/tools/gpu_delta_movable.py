"""lm_delta_movable on a batch of the bench's "movable-lists" shape (bench.py: 16 concurrent sessions over MovableLists — root + child,
nested children, 3 peers, 500 steps, bulk inserts — repeated to fill the batch): the batch is staged and run at the latest version, then
one query per document asks for the MovableList deltas from A = the version recorded in the middle of the document's history.  Reports
k_mldelta_mark + k_mldelta next to the emit stage of the same run (k_emit*: lm_set_profiling(1)) and the bytes lm_delta_movable copies
back (lm_delta_bytes) against the JSON bytes lm_fetch would move.  The answers of the 16 distinct documents are checked against the
plain reference (_delta_movable.py).
Not a test.  usage: python tests/tools/gpu_delta_movable.py [docs]     (one GPU step; run it under `timeout -k 10`)"""
import json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loro_amd

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 4096

if __name__ == "__main__":
    import _delta_movable, _fuzz, _merge_ref
    from _richtext_ref import changes_of
    blobs, models, avv, want = [], [], [], []
    for d in range(16):
        snaps = []
        reps = _fuzz.movable_session(7000 + d, n_peers=3, n_steps=500, sync_prob=0.08, nested=True, bulk=300, snapshots=snaps)
        blobs.append(_fuzz.blobs_of(reps, random.Random(d)))
        m = _merge_ref.Model(changes_of(reps))
        fr = list(snaps[len(snaps) // 2][0])
        models.append(m); avv.append(m.vv(fr))
        want.append(_delta_movable.expected(m, m.version(fr), m.all_ids))
    tot = {k: sum(w[2][k] for w in want) for k in _delta_movable.OUTCOMES}
    print("the 16 documents:", sum(len(m.all_ids) for m in models), "op ids,", sum(len(w[0]) for w in want), "delta bytes,", tot, flush=True)
    out = {"docs": DOCS, "distinct": 16, "op_ids_per_doc_mean": sum(len(m.all_ids) for m in models) // 16}
    with loro_amd.MergeEngine(0) as e:
        e.set_profiling(1)
        res = e.merge_batch([blobs[i % 16] for i in range(DOCS)])
        assert [r[:3] for r in res[:16]] == [m.result()[:3] for m in models]
        out["lm_run_stage_ms"] = {n: round(ms, 3) for n, ms in e.kernel_times()}
        out["k_emit_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_emit")), 3)
        out["k_mlist_post_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_mlist_post")), 3)
        out["json_bytes"] = sum(len(r[1]) for r in res)
        q = [(d, avv[d % 16]) for d in range(DOCS)]
        best = None
        for _ in range(3):
            n0 = len(e.kernel_times())                    # (the stage list grows with every call: this call's entries are its tail)
            t = time.perf_counter()
            got = e.delta_movable(q)
            wall = time.perf_counter() - t
            k = {}
            for n, ms in e.kernel_times()[n0:]:           # (a call that took the overflow path lists k_mldelta twice: summed)
                k[n] = k.get(n, 0.0) + ms
            for d in range(DOCS):
                assert got[d] == (0, want[d % 16][1], want[d % 16][0]), "document %d differs from the reference" % d
            if best is None or sum(k.values()) < sum(best["k"].values()):
                best = {"k": k, "wall": wall, "launches": [n for n, _ in e.kernel_times()[n0:]].count("k_mldelta")}
            out["delta_json_bytes"] = sum(len(g[2]) for g in got)
            out["delta_d2h_bytes"] = int(e.b.delta_bytes(e.h))   # what the call copied back: result rows + the packed answers
        out["k_mldelta_mark_ms"] = round(best["k"].get("k_mldelta_mark", 0.0), 3)
        out["k_mldelta_ms"] = round(best["k"].get("k_mldelta", 0.0), 3)
        out["k_mldelta_launches_all_streams"] = best["launches"]      # (one per stream of the context unless a slab overflowed)
        out["k_delta_pack_ms"] = round(best["k"].get("k_delta_pack", 0.0), 3)
        out["lm_delta_movable_wall_ms"] = round(best["wall"] * 1e3, 1)
        out["k_mldelta_over_k_emit"] = round(out["k_mldelta_ms"] / out["k_emit_ms"], 2) if out["k_emit_ms"] else None
        assert e.fetch() == res
    print(json.dumps(out))
