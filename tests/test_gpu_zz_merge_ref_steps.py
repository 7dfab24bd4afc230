"""GPU: documents that arrive in steps (lm_stage + lm_import + lm_run, the trackers kept in HBM between the steps) and snapshot bases
(lm_snapshot_base.h) on the gfx950 build against the bytes of the plain merge model's `Session` (tests/_merge_ref.py) — the oracle is
only the third column of a failure message.  The sessions are those of tests/test_merge_ref_steps.py (tests/_merge_docs_steps.py):
the four fuzz corpora under the default kernel choice, LM_PLAIN=0 and LM_PART_MIN_DOCS=4 with the fallback cap from the restated
layout / leaf-pool / record rules; every hand-built group with resident_fresh() exact after every run; the snapshot bases as one batch
with state_documents() / redo_documents() exact under six settings, and as resident documents.  Documents and models are built once
per module, one engine serves every test.

Measured on an MI355X, seconds: the module 22.3, of which the fixture (160 fuzz sessions, 21 groups, 38 snapshot bases and their models,
host only) 20.7; test_fuzz_sessions 0.16 / 0.13 / 0.13 (960 step renderings each), test_hand_built_groups 0.21 / 0.21 (21 groups, 1,547
step renderings), the snapshot bases as one batch 0.02 or less per setting, as resident documents 0.14."""
import pytest

import _merge_docs_steps as S, _oracle
import test_merge_ref_steps as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def docs():
    corpora = S.step_corpora()
    S.check_step_conditions(corpora)
    return {"fuzz": corpora, "groups": S.groups(), "bases": S.base_corpus() + S.base_hand_docs()}


@pytest.mark.parametrize("env", T.ENVS, ids=T.ids_of)
def test_fuzz_sessions(engine, docs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pairs = predicted = 0
    for name, ds in docs["fuzz"].items():
        seen = S.run_group(engine, name, ds, what="device %s" % (env or ""))
        per = [S.predicted_fresh(d) for d in ds]
        cap = [sum(x[k] for x in per) for k in range(5)]
        assert seen[0] <= len(ds) and all(s <= m for s, m in zip(seen[1:], cap)), (name, seen, cap)
        pairs += 5 * len(ds); predicted += sum(cap)
    assert predicted * 4 <= pairs, (predicted, pairs)


@pytest.mark.parametrize("env", T.ENVS[:2], ids=T.ids_of)
def test_hand_built_groups(engine, docs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name, genv, ds, fresh in docs["groups"]:
        for k, v in genv.items():
            monkeypatch.setenv(k, v)
        S.run_group(engine, name, ds, fresh, what="device %s" % (dict(env, **genv) or ""))
        assert "LM_DIR_OPT_MAX" not in genv or engine.sizing()[3] >= 1, name
        for k in genv:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("env", T.BASE_ENVS, ids=T.ids_of)
def test_snapshot_bases_as_one_batch(engine, docs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    T.run_bases(engine, docs["bases"], env, "device")


def test_snapshot_bases_as_resident_documents(engine, docs):
    n = max(len(d.steps.steps) for d in docs["bases"])
    ds = [d.steps.padded(n) for d in docs["bases"]]
    S.run_group(engine, "snapshot bases", ds, [len(ds)] + [0] * (n - 1), what="device")
