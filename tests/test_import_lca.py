"""Import mode and common ancestors (k_import_lca) on the kernel-logic harness: the plain-model contract S0-S5, the literal answers of
the hand-built groups and the oracle's Session, step by step (tests/_import_lca.py has the expectation and the documents).
Order: the corpus floors, from the model and the restatement, before any comparison; the oracle's own answers against the contract and
the literals; the restatement against the known answers and the three node partitions against each other; then the harness under
the default setting and under LM_CUT_MIN_ROWS=0 (every document's nodes cut at successors), LM_PART_MIN_DOCS=4 (several streams:
the inv / first mapping of lm_import_modes) and LM_DIR_OPT_MAX=4 (documents that take the retry launch)."""
import os

import pytest

import _emu
import _import_lca as IL
from loro_amd._cabi import Context
from loro_amd import wire

_CACHE = {}


def _docs():
    if "docs" not in _CACHE:
        groups = IL.hand_groups()
        hand = [d for g in groups.values() for d in g]
        docs = hand + IL.corpus()
        _CACHE["groups"], _CACHE["docs"] = groups, docs
        _CACHE["oracle"] = IL.oracle_run(docs)     # computed once, shared, never changed
    return _CACHE["docs"]


def test_decode_frontiers_round_trip():
    for ids in ([], [(7, 4)], [(5, 0), ((1 << 32) + 5, 3), ((1 << 63) + 5, 1 << 20), ((1 << 64) - 1, 0)]):
        assert IL.decode_frontiers(wire.encode_frontiers(ids)) == ids


def test_corpus_floors():
    """before any comparison: the corpus shows what it must, counted from the model and the restatement alone"""
    tot = IL.counts(_docs(), lambda d: [None if e is None else (e[0], wire.encode_frontiers(e[1])) for e in IL.expected(d)])
    print(tot)
    for k, floor in IL.FLOORS.items():
        assert tot[k] >= floor, (k, tot)


def test_the_oracle_keeps_the_contract_and_the_literals():
    """S0-S5 over the ORACLE's answers on everything: were one violated, the contract would be misread.  The literals hold for the
    oracle too, except where they pin the kernel's own limits (more than 16 ancestors, more than 64 heads, more than 256 peers)."""
    docs = _docs()
    orc = _CACHE["oracle"]
    for i, d in enumerate(docs):
        for k, f in enumerate(d.facts()):
            res, info = orc[k][i]
            where = "oracle: %s, step %d" % (d.label, k)
            if k >= d.no_oracle_from:
                continue
            if f.failed:
                assert res[0] not in (0, 4, 6), where
                continue
            IL.check_answer(f, info, where)
            if d.want is not None and k not in d.oracle_differs:
                assert (info[0], IL.decode_frontiers(info[1])) == d.want[k], (where, info, d.want[k])


def test_the_heap_overflow_document_has_an_answer_in_the_reference():
    """what the kernel gives up on ("60 roots under 60 heads", step 1: -1, pinned in its literals) the restatement and the oracle
    answer: Import, []"""
    docs = _docs()
    i = next(i for i, d in enumerate(docs) if d.label == "60 roots under 60 heads")
    assert docs[i].want[1] == IL.UNKNOWN and IL.expected(docs[i])[1] == ("Import", [])
    assert _CACHE["oracle"][1][i][1] == ("Import", wire.encode_frontiers([]))


def _n(peer, counter, length, lamport, deps):
    return (peer, counter, length, lamport, list(deps))


def test_restatement_reproduces_the_known_answers():
    """dag.rs:1108-1276, the node lists of tests/test_oracle_dag.py, without the oracle"""
    f = IL.find_common_ancestor
    d = [_n(1, 0, 2, 0, []), _n(1, 2, 2, 2, [(1, 1)])]
    assert f(d, [], [(1, 3)]) == ([], "Linear")
    assert f(d, [(1, 3)], []) == ([], "Checkout")
    assert f(d, [(1, 0)], [(1, 1)]) == ([(1, 0)], "Linear")
    assert f(d, [(1, 1)], [(1, 0)]) == ([(1, 0)], "Checkout")
    assert f(d, [(1, 1)], [(1, 3)]) == ([(1, 1)], "Linear")
    assert f([_n(1, 1, 1, 1, [(1, 0)])], [], [(1, 1)]) == ([], "ImportGreaterUpdates")
    d = [_n(1, 0, 1, 0, []), _n(2, 0, 1, 1, [(1, 0)]), _n(3, 0, 1, 2, [(1, 0)]), _n(4, 0, 1, 3, [(2, 0), (3, 0)])]
    assert f(d, [(2, 0)], [(3, 0)]) == ([(1, 0)], "Checkout")
    assert f(d, [(1, 0)], [(4, 0)])[0] == [(1, 0)]
    assert f([_n(1, 0, 1, 0, []), _n(2, 0, 1, 1, []), _n(3, 0, 1, 2, [(1, 0), (2, 0)])], [(1, 0)], [(3, 0)]) == ([], "Checkout")
    d = [_n(1, 0, 1, 0, []), _n(2, 0, 1, 1, []), _n(3, 0, 1, 2, []), _n(4, 0, 1, 3, [(1, 0), (2, 0), (3, 0)])]
    assert f(d, [(1, 0), (2, 0)], [(4, 0)]) == ([], "Checkout")
    assert f([_n(1, 0, 1, 0, []), _n(2, 0, 1, 1, [(1, 0)])], [(1, 0)], [(2, 0)]) == ([(1, 0)], "ImportGreaterUpdates")
    d = [_n(1, 0, 1, 0, []), _n(2, 0, 1, 1, [(1, 0)]), _n(3, 0, 1, 2, [(1, 0)]), _n(4, 0, 1, 3, [(2, 0), (3, 0)])]
    assert f(d, [(2, 0)], [(4, 0)]) == ([], "Checkout")
    d = [_n(1, 0, 1, 0, []), _n(2, 0, 2, 1, [(1, 0)]), _n(3, 0, 2, 3, [(1, 0)]), _n(4, 0, 1, 5, [(2, 1), (3, 1)])]
    assert f(d, [(4, 0), (2, 1), (3, 1)], [(2, 0), (3, 0)]) == ([(2, 0), (3, 0)], "Checkout")
    d = [_n(1, 0, 1, 0, []), _n(2, 0, 1, 1, [(1, 0)]), _n(3, 0, 1, 2, [(1, 0)]), _n(4, 0, 1, 3, [(1, 0)])]
    assert f(d, [(2, 0), (3, 0)], [(2, 0), (4, 0)]) == ([(2, 0)], "Checkout")


def test_partitions_agree():
    """the walk runs over DAG nodes, and three partitions of the same history are in play: never cut (the oracle), cut at every
    change with a successor of another peer (k_dag_a for large documents, or all under LM_CUT_MIN_ROWS=0) and the reference's own —
    has_succ and splits in delivery order, pending changes entering when they apply (`_import_lca.Delivered`), which is the
    expectation of every step.  The restatement gives the SAME (mode, L) on all three for every step of the corpus and the
    hand-built groups: 0 disagreements in 1,081 steps.  So the kernel may use either of its two.  (The answer is not independent of
    the partition in general: with every change a node of its own some steps that continue one head's own peer by several changes
    leave the same-peer fast exit, dag.rs:520-546, and come out ImportGreaterUpdates instead of Linear, same L — counted, not a
    partition anybody builds.)  Also checked: every cut of the reference's partition is a cut of the successor partition."""
    n = bad = finer = 0
    for d in _docs():
        for k, f in enumerate(d.facts()):
            if f.failed:
                continue
            got = {name: IL.restated(f, b) for name, b in IL.PARTITIONS.items()}
            n += 1
            if len(set((m, tuple(L)) for m, L in got.values())) != 1:
                bad += 1
                print("partition", d.label, k, got)
            starts = lambda nodes: {(x[0], x[1]) for x in nodes}
            assert starts(IL.never_cut(f.model)) <= starts(f.nodes) <= starts(IL.cut_at_successors(f.model)), (d.label, k)
            fine = IL.restated(f, lambda f: IL.every_change(f.model))
            if fine != got["as_delivered"]:
                finer += 1
                assert fine == ("ImportGreaterUpdates", got["as_delivered"][1]) and got["as_delivered"][0] == "Linear", (d.label, k, fine, got)
    print("steps", n, "disagreements", bad, "with every change a node", finer)
    assert bad == 0 and (n, finer) == (1081, 5)


@pytest.mark.parametrize("env", [{}, {"LM_CUT_MIN_ROWS": "0"}, {"LM_CUT_MIN_ROWS": "1000000"}, {"LM_PART_MIN_DOCS": "4"}, {"LM_DIR_OPT_MAX": "4"}],
                         ids=["default", "cut_all", "cut_none", "streams", "retry"])
def test_harness(env):
    docs = _docs()
    os.environ.update(env)
    try:
        got = IL.run(lambda: Context(_emu.binding()), docs)
    finally:
        for k in env:
            del os.environ[k]
    IL.check_run(docs, got, oracle=_CACHE["oracle"], what="harness " + str(env))


def test_after_a_failure_alone():
    """the group of the fix as a batch of its own (document 0 of a batch fails, document 1 does not: each keeps its own `from`)"""
    docs = IL.after_a_failure()
    got = IL.run(lambda: Context(_emu.binding()), docs)
    IL.check_run(docs, got, oracle=IL.oracle_run(docs), what="harness")


def test_api_edges():
    IL.api_edges(lambda: Context(_emu.binding()))
