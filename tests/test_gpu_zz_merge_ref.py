"""GPU: the bytes of the gfx950 build against the bytes of the plain merge model (tests/_merge_ref.py) — the oracle is only the third
column of a failure message.  The fuzz corpora of tests/test_merge_ref.py at the latest version and at checkouts under the default
kernel choice, LM_SPAN=0, LM_PLAIN=0 and LM_CUT_MIN_ROWS=0, and hand-built documents aimed at the integrate kernels' edges
(tests/_merge_docs.py): three-peer texts of 70 / 130 / 300 runs with concurrent inserts in every leaf's first and last slot (once
with the optimistic directory forced down to four entries), two-peer documents whose concurrent branch lies just below / just past
the leaf-sweep threshold, a linear prefix handed to concurrent branches, edits that straddle the 16-aligned ids loc[] keeps, and
backspace runs cut by checkouts.  The models are built once per module.

Measured on an MI355X, seconds: the module 7.7, of which the fixture (corpora, hand-built documents and their models, host only) 6.7;
test_fuzz_corpora 0.11 / 0.08 / 0.06 / 0.06 (480 renderings each), test_three_peer_texts 0.06 (three batches), the leaf-sweep documents
0.03 and 0.02 (240 renderings each), the linear prefix 0.02, id windows + backspace runs 0.01 each."""
import pytest

import _merge_docs, _oracle
from loro_amd import wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import loro_amd
    e = loro_amd.MergeEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def docs():
    out = _merge_docs.corpora()
    for name, ds in out.items():
        _merge_docs.check_conditions(name, ds)
    out = {"fuzz": [d for ds in out.values() for d in ds]}
    out["three"] = [_merge_docs.three_peer_text(n, n) for n in (70, 130, 300)]
    out["sweep"] = _merge_docs.sweep_docs()
    out["linear"] = _merge_docs.linear_prefix_docs()
    out["windows"] = _merge_docs.id_window_docs()
    out["backspace"] = _merge_docs.backspace_docs()
    return out


def run(engine, ds, what, n_versions=2):
    """the documents at the latest version and at `n_versions` of their versions, one batch; every result against the model's"""
    at = [(d, None) for d in ds] + [(d, fr) for d in ds for fr in d.versions[:n_versions]]
    blobs = [d.blobs for d, _ in at]
    fronts = [None if fr is None else wire.encode_frontiers(fr) for _, fr in at]
    got = engine.merge_batch(blobs, fronts)
    assert len(got) == len(at)
    for (d, fr), b, f, g in zip(at, blobs, fronts, got):
        w = d.model.result(fr)
        if g != w:
            raise AssertionError("%s %s at %s:\n device %r\n model  %r\n oracle %r" % (what, d.label, fr, g[:3], w[:3], _oracle.merge(b, frontiers=f)[:3]))
    return len(at)


@pytest.mark.parametrize("env", [{}, {"LM_SPAN": "0"}, {"LM_PLAIN": "0"}, {"LM_CUT_MIN_ROWS": "0"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_fuzz_corpora(engine, docs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert run(engine, docs["fuzz"], env) >= 3 * 160


def test_three_peer_texts(engine, docs, monkeypatch):
    run(engine, docs["three"], "three peers", n_versions=6)
    monkeypatch.setenv("LM_DIR_OPT_MAX", "4")
    run(engine, docs["three"], "three peers, LM_DIR_OPT_MAX=4", n_versions=6)
    assert engine.sizing()[3] >= 1
    monkeypatch.setenv("LM_SPAN", "0")
    run(engine, docs["three"], "three peers, LM_DIR_OPT_MAX=4, LM_SPAN=0", n_versions=6)
    assert engine.sizing()[3] >= 1


@pytest.mark.parametrize("plain", ["2", "0"])
def test_retreat_by_leaf_sweep(engine, docs, monkeypatch, plain):
    monkeypatch.setenv("LM_PLAIN", plain)
    run(engine, docs["sweep"], "LM_PLAIN=" + plain)


def test_linear_prefix_handed_to_concurrent_branches(engine, docs, monkeypatch):
    monkeypatch.setenv("LM_CUT_MIN_ROWS", "0")
    run(engine, docs["linear"], "LM_CUT_MIN_ROWS=0", n_versions=4)


@pytest.mark.parametrize("span", ["1", "0"])
def test_id_windows_and_backspace_runs(engine, docs, monkeypatch, span):
    monkeypatch.setenv("LM_SPAN", span)
    run(engine, docs["windows"], "LM_SPAN=" + span, n_versions=4)
    run(engine, docs["backspace"], "LM_SPAN=" + span, n_versions=6)
