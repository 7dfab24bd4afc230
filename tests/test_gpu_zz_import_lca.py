"""Import mode and common ancestors on the device (k_import_lca through the C ABI): the hand-built groups and the corpus of
tests/_import_lca.py as ONE batch of several hundred resident documents per step — different answers side by side in the kernel's
output and scratch — under the default setting, LM_CUT_MIN_ROWS=0, LM_PART_MIN_DOCS=4 and LM_DIR_OPT_MAX=4.  Every (mode, L) is held
against the plain-model contract S0-S5, the literals of the hand-built documents and the oracle's Session, all computed on the host
once per module."""
import os

import pytest

import _import_lca as IL
import test_import_lca as T

pytestmark = pytest.mark.gpu

_CACHE = {}


def _engine():
    import loro_amd
    return loro_amd.MergeEngine(0)


def _batch():
    if not _CACHE:
        docs = T._docs()
        n_hand = sum(len(g) for g in T._CACHE["groups"].values())
        docs = docs + docs[n_hand:]                     # the corpus twice: more than 256 documents, both streams of a context
        orc = T._CACHE["oracle"]
        _CACHE["docs"], _CACHE["oracle"] = docs, [row + row[n_hand:] for row in orc]
    return _CACHE["docs"], _CACHE["oracle"]


@pytest.mark.parametrize("env", [{}, {"LM_CUT_MIN_ROWS": "0"}, {"LM_PART_MIN_DOCS": "4"}, {"LM_DIR_OPT_MAX": "4"}],
                         ids=["default", "cut_all", "streams", "retry"])
def test_device(env):
    docs, orc = _batch()
    assert len(docs) > 256
    os.environ.update(env)
    try:
        got = IL.run(_engine, docs)
    finally:
        for k in env:
            del os.environ[k]
    IL.check_run(docs, got, oracle=orc, what="device " + str(env))


def test_after_a_failure_on_the_device():
    docs = IL.after_a_failure()
    IL.check_run(docs, IL.run(_engine, docs), oracle=IL.oracle_run(docs), what="device")


def test_api_edges_on_the_device():
    IL.api_edges(_engine)
