"""GPU: the bytes of the gfx950 build against the bytes of the plain merge model (tests/_merge_ref.py) for LWW Map documents decoded
WITHOUT op rows (k_map_fused, lm_k_map_fused.h) — the oracle is only the third column of a failure message.  The documents of
tests/test_merge_ref_map.py (tests/_merge_docs_map.py: fuzz corpora as incremental blobs and as whole exports, hand-built groups that
know whether the kernel decides them or hands them over) under the same five settings — k_map_fused forced on, LM_MAP_FUSED=0,
LM_LWW_LDS=0, LM_HT_OPT=64, LM_DECODE=0 — checkouts with LM_SHARE_REPLAY=0, and the RACE documents no harness can show: 32 and 65
blocks of 1,024 rows by 16 peers on 1, 2, 4 and 1,000 keys, every lamport shared by 16 writes, each document 38 times in the batch
(304 workgroups in flight) with k_map_fused forced on, and the two 1,000-key ones under the other four settings.  Every batch asserts fused_documents and redo_documents exactly.  One engine and one set of models per module.

Measured on an MI355X, seconds: the module 18, of which the fixtures (host only) 1.4 for the corpora, the hand-built documents and
their models and 4.2 for the race documents (eight histories of 33k / 67k rows); test_sixteen_waves_race_for_one_table 5.6 with
k_map_fused forced on (304 entries, 85 MB of blobs staged) and 1.3 - 1.4 under each other setting (76 entries); test_hand_built_documents 0.10 - 0.12 per setting (27 batches, 441 renderings);
test_fuzz_corpora 0.03 - 0.09 per setting (600 renderings)."""
import pytest

import _merge_docs_map as M, _oracle

pytestmark = pytest.mark.gpu


def oracle(blobs, fronts):
    return _oracle.merge(blobs, frontiers=fronts)


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def docs():
    corpora = M.map_corpora()
    for name, ds in corpora.items():
        M.check_map_conditions(name, ds)
    fuzz = [d for ds in corpora.values() for d in ds]
    return {"fuzz": fuzz, "whole": [d.whole_exports() for d in fuzz], "groups": M.hand_built() + M.table_docs(64)}


@pytest.fixture(scope="module")
def races():
    return M.race_docs()


def under(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LM_SHARE_REPLAY", "0")


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_fuzz_corpora(engine, docs, monkeypatch, setting):
    name, env, fused_on, ht_opt = setting
    under(monkeypatch, env)
    n = M.run_group(engine, "corpora", M.STAYS, docs["fuzz"], oracle, name, max_versions=M.RUN_VERSIONS, fused_on=fused_on, ht_opt=ht_opt)
    n += M.run_group(engine, "corpora", M.STAYS, docs["whole"], oracle, name, max_versions=0, fused_on=fused_on, ht_opt=ht_opt)
    assert n == (2 + M.RUN_VERSIONS) * len(docs["fuzz"])      # (every corpus document has ten versions at least)


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_hand_built_documents(engine, docs, monkeypatch, setting):
    name, env, fused_on, ht_opt = setting
    under(monkeypatch, env)
    n = 0
    for label, path, ds in docs["groups"]:
        n += M.run_group(engine, label, path, ds, oracle, name, fused_on=fused_on, ht_opt=ht_opt)
    assert n == M.n_renderings(docs["groups"])


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_sixteen_waves_race_for_one_table(engine, races, monkeypatch, setting):
    """k_map_fused forced on: all eight documents, 38 times each — 304 workgroups of 16 waves.  The other four settings take the two
    1,000-key documents (38 times each, 76 entries): the same contention for table slots in the row-table LWW kernels (LDS and HBM),
    and under LM_HT_OPT=64 in k_map_fused until the 33rd claim, after which every entry is handed over"""
    name, env, fused_on, ht_opt = setting
    under(monkeypatch, env)
    (label, path, ds), = races
    if name != "fused":
        ds = [d for d in ds if d.model.map_pairs() == 1000]
        assert len(ds) == 2
    n = M.run_group(engine, label, path, ds, oracle, "races, " + name, repeat=38, fused_on=fused_on, ht_opt=ht_opt)
    assert n == 38 * len(ds) and (name != "fused" or n >= 300)
