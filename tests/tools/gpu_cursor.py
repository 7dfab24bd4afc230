"""lm_cursor_pos on configs[1] documents (BASELINE.json: 100k-op trace, two concurrent peers): k_cursor's time for 8 and for 256
queries per document next to the same batch's emit stage (lm_set_profiling(1)) — both make one pass over the same leaves.
Not a test.  usage: python tests/tools/gpu_cursor.py [docs] [base_ops] [branch_ops]     (one GPU step; run it under `timeout -k 10`)"""
import json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loro_amd
from loro_amd import workload, wire

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
N_BASE = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
N_BRANCH = int(sys.argv[3]) if len(sys.argv) > 3 else 25000
TEXT = "cid:root-text:Text"

if __name__ == "__main__":
    import _cursor
    tpl = workload.Cfg2Template(N_BASE, N_BRANCH, seed=0, commit_every=10, fuse=True)
    docs = [tpl.stamp(d) for d in range(DOCS)]
    ex = _cursor.Expect(docs[0], docs[0], "text", wire.KIND_TEXT)            # document 0's answers: the parity check of the timed calls
    pa = (0 * 2 + 1) * 0x9E3779B1 % (1 << 53) | 1
    print("generated", DOCS, "documents;", len(ex.order), "ids,", len(ex.visible), "visible", flush=True)
    rng = random.Random(0)
    # ids by (peer A = base + its branch | peer B, counter): the same counters name elements in every stamped document
    tomb = [i for i in ex.order if i not in ex.vis]
    picks = [rng.choice(tomb if k % 4 == 3 else ex.visible) for k in range(256)]     # every fourth one a tombstone

    def peers_of(d):
        a = (d * 2 + 1) * 0x9E3779B1 % (1 << 53) | 1
        return {pa: a, pa + 1: a + 1}
    out = {"docs": DOCS, "ops_per_doc": N_BASE + 2 * N_BRANCH}
    with loro_amd.MergeEngine(0) as e:
        e.set_profiling(1)
        e.stage(docs); e.run()
        emit = sum(ms for n, ms in e.kernel_times() if n.startswith("k_emit"))
        out["k_emit_ms_with_linear_prefix"] = round(emit, 3)
        t = time.perf_counter(); e.cursor_pos([(0, TEXT, picks[0], 0)]); out["first_call_s_incl_rerun_without_linear_prefix"] = round(time.perf_counter() - t, 3)
        e.run()
        out["k_emit_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_emit")), 3)
        out["lm_run_stage_ms"] = {n: round(ms, 3) for n, ms in e.kernel_times()}
        import ctypes
        import numpy as np
        from loro_amd._cabi import CursorQuery, CursorResult
        qdt = np.dtype([("doc", "<u8"), ("container", "<u8"), ("container_len", "<u8"), ("has_id", "<i4"), ("peer", "<u8"), ("counter", "<i4"), ("side", "<i4")], align=True)
        assert qdt.itemsize == ctypes.sizeof(CursorQuery)
        key = ctypes.create_string_buffer(TEXT.encode())
        peer_a = np.array([peers_of(d)[pa] for d in range(DOCS)], dtype=np.uint64)
        for nq in (8, 256):
            # the queries as the C caller holds them (packed once, outside the timed call)
            is_b = np.array([p != pa for p, _ in picks[:nq]], dtype=np.uint64)
            q = np.zeros(DOCS * nq, dtype=qdt)
            q["doc"] = np.repeat(np.arange(DOCS, dtype=np.uint64), nq)
            q["container"] = ctypes.addressof(key); q["container_len"] = len(TEXT); q["has_id"] = 1
            q["peer"] = np.repeat(peer_a, nq) + np.tile(is_b, DOCS)
            q["counter"] = np.tile(np.array([c for _, c in picks[:nq]], dtype=np.int32), DOCS)
            r = (CursorResult * (DOCS * nq))()
            best_wall, best_k = 1e9, 1e9
            for _ in range(3):
                t = time.perf_counter()
                rc = e.b.cursor_pos(e.h, ctypes.cast(q.ctypes.data, ctypes.POINTER(CursorQuery)), DOCS * nq, r)
                wall = time.perf_counter() - t
                assert rc == 0, e.b.last_error(e.h)
                k = sum(ms for n, ms in e.kernel_times() if n == "k_cursor")
                e.run()                                   # (clears the stage list: the next call's k_cursor entries stand alone)
                best_wall, best_k = min(best_wall, wall), min(best_k, k)
            got = [(x.status, x.pos, x.pos_utf16, x.side) for x in (r[i] for d in range(0, DOCS, max(1, DOCS // 50)) for i in range(d * nq, (d + 1) * nq))]
            want = [ex.pos_answer(i, 0) for i in picks[:nq]]
            assert got[:nq] == want, "document 0 differs from the oracle"
            assert all(got[k * nq:(k + 1) * nq] == want for k in range(len(got) // nq)), "stamped documents differ"
            out["q%d" % nq] = {"k_cursor_ms": round(best_k, 3), "lm_cursor_pos_wall_ms": round(best_wall * 1e3, 1),
                               "deleted": sum(1 for w in want if w[0] == 1), "ok": sum(1 for w in want if w[0] == 0)}
    print(json.dumps(out))
