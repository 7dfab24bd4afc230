"""LWW Map documents decoded WITHOUT op rows (k_map_fused, lm_k_map_fused.h) against the plain merge model (tests/_merge_ref.py): until
now the kernel's only reference was the oracle, on documents whose edges the fallback (DF_REDO) could hide.  Documents:
tests/_merge_docs_map.py — fuzz corpora (1-6 peers, root and child Maps, every scalar kind, deletes, syncs; incremental blobs and whole
exports) that must first show what the LWW rule had to decide (check_map_conditions), and hand-built groups that each know whether
k_map_fused decides them or hands them over.  Three comparisons:
  (a) the model against the oracle on every document and version (and the model's pending-change part on the existing pending cases);
  (b) the model against the kernel-logic harness with k_map_fused forced on (LM_MF_MIN_ROWS=1, LM_MF_CHG_RATIO=0);
  (c) the same documents through the other Map paths, each against the model: LM_MAP_FUSED=0, LM_LWW_LDS=0, LM_HT_OPT=64, LM_DECODE=0.
Every batch asserts fused_documents and redo_documents EXACTLY; checkouts run with LM_SHARE_REPLAY=0, so that checked-out entries go
through the fused kernel too.  No document is left out of any comparison.  The race documents (16 waves on one table) are GPU only:
the harness runs its fibers one after the other.

Time, one process on an 8-thread host: the module about two minutes (118 - 133 s) — corpora, hand-built documents and their models 5 s, (a) 4 s, the corpora on the
harness (600 renderings per setting) 21 - 23 s under each of the three settings that leave k_map_fused on and 4 s under the two that
do not, the hand-built groups (27 batches, 441 renderings) 9 - 10 s and 2 s.  Each setting is a test of its own, so pytest-xdist spreads them."""
import pytest

import _cases, _emu, _merge_docs_map as M, _merge_ref, _oracle
from _richtext_ref import changes_of
from loro_amd import wire
from loro_amd._cabi import Context


def oracle(blobs, fronts):
    return _oracle.merge(blobs, frontiers=fronts)


@pytest.fixture(scope="module")
def corpora():
    out = M.map_corpora()
    for name, docs in out.items():
        M.check_map_conditions(name, docs)
    return out


@pytest.fixture(scope="module")
def groups():
    return M.hand_built() + M.table_docs(64)


def against_oracle(docs, what):
    at = [(d, None) for d in docs] + [(d, fr) for d in docs for fr in d.versions]
    got = _oracle.merge_batch([d.blobs for d, _ in at], threads=8, frontiers=[None if fr is None else wire.encode_frontiers(fr) for _, fr in at])
    for (d, fr), g in zip(at, got):
        assert g == d.model.result(fr), (what, d.label, fr, g[:3], d.model.result(fr)[:3])
    return len(at)


# ------------------------------------------------------------------------------------------------------------ the model's own parts
def test_limits_are_the_sources():
    """the documents' sides come from the constants of the source text: MF_KMAX, MF_RMAX, 32 containers, half the table, 0xfff0, MAX_PEERS.
    The check of the source text itself is the string asserts inside _merge_docs_map.limits(), which run when that module is imported:
    a limit written differently in the source fails every test of this module at collection.  Here: which limits the documents use, and
    the host's table sizes they were worked out from."""
    assert set(M.LIMITS) == {"MF_KMAX", "MF_RMAX", "MAX_PEERS", "LWW_LDS_CAP", "SECTION", "CONTAINERS"}
    assert M.table_cap(3000) == M.LIMITS["LWW_LDS_CAP"] and M.table_cap(100, 64) == 64 and M.table_cap(100) == 256


def test_applied_set_is_a_fixpoint_whatever_the_order():
    a, b = wire.Replica(1), wire.Replica(2)
    a.map_set("m", "k", 1); a.commit()
    b.merge_from(a)
    b.map_set("m", "k", 2); b.commit()
    a.merge_from(b)
    a.map_set("m", "k", 3); a.commit()
    c1, c3 = a.changes[1]
    c2 = b.changes[2][0]
    for order in ([c3, c2, c1], [c1, c2, c3], [c2, c3, c1]):
        assert _merge_ref.applied_ends(order) == {1: 2, 2: 1}
    assert _merge_ref.applied_ends([c3, c2]) == {} and _merge_ref.applied_ends([c1, c3]) == {1: 1}
    m = _merge_ref.Model([c1, c2, c3], delivered=[c1, c3])
    assert m.result() == (0, b'{"m":{"k":1}}', wire.encode_vv({1: 1}), 1)
    m = _merge_ref.Model([c1, c2, c3], delivered=[c3, c2])
    assert m.result() == (0, b"{}", wire.encode_vv({}), 2)


def test_pending_changes_against_the_oracle_on_the_existing_cases():
    """_cases.edge_case_docs "pending only" / "pending resolved later" (and the duplicated blobs that apply): the writer restated here"""
    names, docs = _cases.edge_case_docs()
    by = dict(zip(names, docs))
    a = wire.Replica(1); a.text_insert("text", 0, "ab"); a.commit()
    a.text_insert("text", 2, "cd"); a.commit()
    first, second = a.changes[1]
    assert by["pending only"] == [a.export({1: 2})]
    for name, delivered in (("pending only", [second]), ("pending resolved later", [second, first]), ("duplicate blob", [first, first, second, second])):
        m = _merge_ref.Model(changes_of([a]), delivered=delivered)
        assert _oracle.merge(by[name]) == m.result(), name
    assert _merge_ref.Model(changes_of([a]), delivered=[second]).result() == (0, b"{}", wire.encode_vv({}), 2)


def test_map_outcomes_on_a_known_history():
    a, b = wire.Replica(5), wire.Replica(9)
    a.map_set("m", "tie", "a"); a.map_set("m", "gone", 1); a.map_set("m", "alone", 1); a.commit()
    kid = b.map_set_container("m", "kid", wire.KIND_MAP); b.map_delete("m", "gone"); b.commit()
    a.map_set("m", "x", 0); a.map_set("m", "kid", "plain"); a.commit()     # lamport 4 against the child's 0: the child is hidden
    b.map_set("m", "tie", "late"); b.commit()                              # lamport 2 against 0, unseen by a: concurrent, no tie
    m = _merge_ref.Model(changes_of([a, b]))
    assert m.value() == {"m": {"tie": "late", "alone": 1, "x": 0, "kid": "plain"}}
    got = m.map_outcomes(delivery=[5, 9], versions=[[(5, 0)], [(9, 0)]])
    assert got == {"concurrent_keys": 3, "tie_on_lamport": 1, "tie_won_by_last_delivered": 1, "tie_won_by_first_delivered": 0, "winner_is_delete": 1,
                   "child_map_hidden": 1, "checkout_winner_differs": 2}, got
    assert m.map_outcomes(delivery=[9, 5])["tie_won_by_first_delivered"] == 1 and m.map_pairs() == 5 and m.map_pairs([(5, 0)]) == 1


# ------------------------------------------------------------------------------------------------------- (a) the model against the oracle
@pytest.mark.parametrize("name", ["2 peers", "4 peers", "1-6 peers"])
def test_model_against_oracle(corpora, name):
    docs = corpora[name]
    n = against_oracle(docs, name) + against_oracle([d.whole_exports() for d in docs], name)
    assert n == 2 * sum(1 + len(d.versions) for d in docs) and all(len(d.versions) >= M.RUN_VERSIONS for d in docs)


def test_hand_built_documents_against_oracle(groups):
    n = 0
    for label, path, docs in groups:
        if path == "refused":      # (one peer more than the DEVICE takes: the oracle renders it, and so does the model)
            assert _oracle.merge(docs[0].blobs) == docs[0].model.result()
        n += against_oracle(docs, label)
    assert n == M.n_renderings(groups)


# ------------------------------------------------------------------------------------- (b), (c) the model against the kernel-logic harness
def under(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LM_SHARE_REPLAY", "0")


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_corpora_against_harness(corpora, monkeypatch, setting):
    name, env, fused_on, ht_opt = setting
    under(monkeypatch, env)
    docs = [d for ds in corpora.values() for d in ds]
    with Context(_emu.binding()) as c:
        n = M.run_group(c, "corpora", M.STAYS, docs, oracle, name, max_versions=M.RUN_VERSIONS, fused_on=fused_on, ht_opt=ht_opt)
        n += M.run_group(c, "corpora", M.STAYS, [d.whole_exports() for d in docs], oracle, name, max_versions=0, fused_on=fused_on, ht_opt=ht_opt)
    assert n == (2 + M.RUN_VERSIONS) * len(docs)      # (every corpus document has ten versions at least: none is short of two)


def test_key_start_candidates_count_against_MF_KMAX_before_they_are_verified(groups, monkeypatch):
    """what the documents found: the key-start scan bails on more than MF_KMAX bytes below 0x20, keys or not — 300 keys with four tabs
    each are handed over (and replayed right), 300 keys with four spaces each stay; lm_k_map_fused.h says so since"""
    under(monkeypatch, M.FORCE)
    tabs, = [docs for label, path, docs in groups if label == "more control characters than MF_KMAX"]
    spaces = [d for label, path, docs in groups if label == "keys" for d in docs if d.label == "300 keys of four spaces each"]
    assert M.n_table_keys(tabs[0].reps[0]) == M.n_table_keys(spaces[0].reps[0]) == 301 < M.LIMITS["MF_KMAX"]
    with Context(_emu.binding()) as c:
        assert M.run_group(c, "tabs", M.LEAVES, tabs, oracle) == 1 and M.run_group(c, "spaces", M.STAYS, spaces, oracle) == 1


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_hand_built_documents_against_harness(groups, monkeypatch, setting):
    name, env, fused_on, ht_opt = setting
    under(monkeypatch, env)
    n = 0
    with Context(_emu.binding()) as c:
        for label, path, docs in groups:
            n += M.run_group(c, label, path, docs, oracle, name, fused_on=fused_on, ht_opt=ht_opt)
    assert n == M.n_renderings(groups)
