"""GPU: the bytes of the gfx950 build against the bytes of the plain merge model's MovableList rules (tests/_merge_ref.py) — the oracle
is only the third column of a failure message.  The MovableList corpora of tests/test_merge_ref_movable.py (writers' views from the
model) at the latest version and at checkouts under the default kernel choice, LM_SPAN=0 and LM_DIR_OPT_MAX=4, the same documents
delivered as overlapping whole exports, and the hand-built documents of tests/_merge_docs.py: lamport ties decided by peer id (ids on
both sides of 2^32 and 2^63, delivery order unlike id order), a move against a delete, changes of 63 / 64 / 65 / 129 move rows
(k_mlist_post's 64-row passes), 1,500 elements each moved and set (two hash-table keys per element, many leaves; once with the
optimistic directory forced down to four entries), checkouts that split the position / value maxima, children that follow their
element.  The documents and their models are built once per module.

Measured on an MI355X, seconds: the module 6.7, of which the fixture (corpora, hand-built documents and their models, host only) 5.5;
test_fuzz_corpora 0.15 / 0.13 / 0.10 (690 + 90 renderings each), test_table_load_and_many_leaves 0.18 (three batches),
test_row_passes_split_maxima_and_children 0.04 and 0.03, test_lamport_ties_and_move_against_delete 0.01 each."""
import pytest

import _merge_docs
from test_gpu_zz_merge_ref import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def docs():
    corpora = _merge_docs.movable_corpora()
    for name, ds in corpora.items():
        _merge_docs.check_conditions(name, ds)
    out = {"fuzz": [d for ds in corpora.values() for d in ds]}
    out["overlapping"] = _merge_docs.overlapping_docs([d for ds in corpora.values() for d in ds[:10]])
    out["ties"] = _merge_docs.lamport_tie_docs()
    out["delete"], _ = _merge_docs.move_against_delete_docs()
    out["passes"] = _merge_docs.row_pass_docs()
    out["load"] = [_merge_docs.table_load_doc()]
    split, at, want = _merge_docs.split_maxima_docs()
    for name, value in want.items():          # the known values, on the model: what the device is then held to
        assert split.model.value(at.get(name)) == {"ml": value}, name
    out["split"] = [split]
    out["children"], want = _merge_docs.children_docs()
    assert [d.model.value() for d in out["children"]] == [{"ml": w} for w in want]
    return out


@pytest.mark.parametrize("env", [{}, {"LM_SPAN": "0"}, {"LM_DIR_OPT_MAX": "4"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_fuzz_corpora(engine, docs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert run(engine, docs["fuzz"], env) >= 3 * 230
    run(engine, docs["overlapping"], (env, "whole exports"))


@pytest.mark.parametrize("span", ["1", "0"])
def test_lamport_ties_and_move_against_delete(engine, docs, monkeypatch, span):
    monkeypatch.setenv("LM_SPAN", span)
    run(engine, docs["ties"], "LM_SPAN=" + span, n_versions=99)
    run(engine, docs["delete"], "LM_SPAN=" + span, n_versions=99)


@pytest.mark.parametrize("span", ["1", "0"])
def test_row_passes_split_maxima_and_children(engine, docs, monkeypatch, span):
    monkeypatch.setenv("LM_SPAN", span)
    run(engine, docs["passes"], "LM_SPAN=" + span, n_versions=99)
    run(engine, docs["split"], "LM_SPAN=" + span, n_versions=99)
    run(engine, docs["children"], "LM_SPAN=" + span, n_versions=99)


def test_table_load_and_many_leaves(engine, docs, monkeypatch):
    run(engine, docs["load"], "default", n_versions=3)
    monkeypatch.setenv("LM_DIR_OPT_MAX", "4")
    run(engine, docs["load"], "LM_DIR_OPT_MAX=4", n_versions=3)
    assert engine.sizing()[3] >= 1
    monkeypatch.setenv("LM_SPAN", "0")
    run(engine, docs["load"], "LM_DIR_OPT_MAX=4, LM_SPAN=0", n_versions=3)
    assert engine.sizing()[3] >= 1
