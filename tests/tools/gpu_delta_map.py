"""lm_delta_map on configs[2]-shaped RESIDENT documents (BASELINE.json: LWW Map, 16 fully concurrent peers x 10,000 writes on 1,024
keys): the first half of the peers' blobs is the base, staged and run; the other half is imported and run; then one query per
document asks for the Map delta from the end of the base to the latest version.  Reports k_mdelta_mark + k_mdelta next to the Map
part of the same run's stages (k_map_lww, k_emit: lm_set_profiling(1)) and the bytes lm_delta_map copies back (lm_delta_bytes)
against the JSON bytes lm_fetch would move.  Document 0's answer is checked against the plain reference (_delta_map.py).
Not a test.  usage: python tests/tools/gpu_delta_map.py [docs] [peers] [writes] [keys]     (one GPU step; run it under `timeout -k 10`)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loro_amd
from loro_amd import wire, workload

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
PEERS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
WRITES = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
KEYS = int(sys.argv[4]) if len(sys.argv) > 4 else 1024

if __name__ == "__main__":
    import _delta_map, _merge_ref
    blobs = workload.cfg3_doc(0, n_peers=PEERS, n_writes=WRITES, n_keys=KEYS, combined=False)      # one history, every document holds it
    base, rest = blobs[:PEERS // 2], blobs[PEERS // 2:]
    # the model of the same history (cfg3_doc's writers, rebuilt: it returns blobs only)
    reps = []
    for p in range(PEERS):
        r = wire.Replica(p + 1)
        x = (p * 104729 + 1) & 0xFFFFFFFFFFFFFFFF
        for i in range(WRITES):
            x = workload._xorshift64(x)
            r.map_set("map", "key_%d" % (x % KEYS), int(x >> 20) - (1 << 42))
            if (i + 1) % 100 == 0:
                r.commit()
        r.commit()
        reps.append(r)
    assert [r.export() for r in reps] == blobs
    model = _merge_ref.Model([c for r in reps for c in r.changes[r.peer]])
    a_vv = {r.peer: r.vv[r.peer] for r in reps[:PEERS // 2]}
    want, oc, counts = _delta_map.expected(model, _delta_map.vv_ids(a_vv), model.all_ids)
    print("document 0's delta:", len(want), "bytes", counts, flush=True)
    out = {"docs": DOCS, "ops_per_doc": PEERS * WRITES, "keys": KEYS}
    with loro_amd.MergeEngine(0) as e:
        e.set_profiling(1)
        e.stage([base] * DOCS); e.run()
        vv1 = [r[2] for r in e.fetch()]
        assert vv1[0] == wire.encode_vv(a_vv)
        e.import_more([rest] * DOCS); e.run()
        out["lm_run_stage_ms"] = {n: round(ms, 3) for n, ms in e.kernel_times()}
        out["k_map_lww_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_map_lww")), 3)
        out["k_emit_ms"] = round(sum(ms for n, ms in e.kernel_times() if n.startswith("k_emit")), 3)
        res = e.fetch()
        assert res[0][:3] == model.result()[:3]
        out["json_bytes"] = sum(len(r[1]) for r in res)
        q = [(d, vv1[d]) for d in range(DOCS)]
        best = None
        for _ in range(3):
            n0 = len(e.kernel_times())                    # (the stage list grows with every call: this call's entries are its tail)
            t = time.perf_counter()
            got = e.delta_map(q)
            wall = time.perf_counter() - t
            k = {}
            for n, ms in e.kernel_times()[n0:]:           # (a call that took the overflow path lists k_mdelta twice: summed)
                k[n] = k.get(n, 0.0) + ms
            assert got[0] == (0, oc, want), "document 0 differs from the reference"
            assert all(g == got[0] for g in got), "equal documents differ"
            if best is None or sum(k.values()) < sum(best["k"].values()):
                best = {"k": k, "wall": wall, "launches": [n for n, _ in e.kernel_times()[n0:]].count("k_mdelta")}
            out["delta_json_bytes"] = sum(len(g[2]) for g in got)
            out["delta_d2h_bytes"] = int(e.b.delta_bytes(e.h))   # what the call copied back: result rows + the packed answers
        out["k_mdelta_mark_ms"] = round(best["k"].get("k_mdelta_mark", 0.0), 3)
        out["k_mdelta_ms"] = round(best["k"].get("k_mdelta", 0.0), 3)
        out["k_mdelta_launches_all_streams"] = best["launches"]      # (one per stream of the context unless a slab overflowed)
        out["k_delta_pack_ms"] = round(best["k"].get("k_delta_pack", 0.0), 3)
        out["lm_delta_map_wall_ms"] = round(best["wall"] * 1e3, 1)
        assert e.fetch() == res
    print(json.dumps(out))
