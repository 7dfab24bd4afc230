"""The plain merge model's `Session` (tests/_merge_ref.py: a document delivered in steps — applied set, pending changes, the two versions a
step stands at, sticky container states) against
  (a) the known answers of tests/test_emu_resident.py::test_two_imports_are_not_one_import_batch, written here as literals;
  (b) the oracle's Session, step by step, on every session of tests/_merge_docs_steps.py (fuzz and hand-built);
  (c) the kernel-logic harness: lm_stage + lm_import + lm_run with the trackers kept between the steps, under the default kernel choice,
      LM_PLAIN=0 and LM_PART_MIN_DOCS=4 (LM_SPAN=0 is refused for resident documents by the host — asserted — and runs on the snapshot
      bases as a batch), with resident_fresh() EXACT after every run of every hand-built group and capped for the fuzz sessions by the
      layout / leaf-pool / record rules restated over the inputs (_merge_docs_steps.Layout);
  (d) snapshot bases (lm_snapshot_base.h) as one batch — state_documents() and redo_documents() exact under six settings — and as
      resident documents, against the model that stands at the base version and then takes the updates.
A failure names the session, the step and three columns: kernel, model, oracle.

Found by (c): a resident MovableList document whose step brought a peer that sorts in front of the stored ones rendered a wrong list
("a,d,b,e" for "a,c,d,b,e"): the id a move keeps of the item it deleted is a (peer index, counter) pair in cp[], the renumbering of the
stored leaves does not reach it, and the retreat of that move took its delete back from another peer's item.  Such a document is now
replayed from the empty version (lm_k_integrate_span.h, `lost`); pinned by the "movable list" and "new peers, ml" groups.

Time.  140 s for the module in one process on an 8-thread host: the fixture (160 fuzz sessions, 21 groups, 38 snapshot bases and their
models — a session's model is rebuilt at every step) 48 s, (b) 0.5 s, and the harness 91 s: the fuzz sessions 3 x 11 s (960 step renderings
each), the groups 3 x 17 s (1,547 each), the snapshot bases 6 x 0.8 s as batches and 2 s as resident documents."""
import os, re

import pytest

import _emu, _merge_docs_steps as S, _merge_ref, _oracle
from loro_amd import wire
from loro_amd._cabi import Context

ENVS = [{}, {"LM_PLAIN": "0"}, {"LM_PART_MIN_DOCS": "4"}]
ids_of = lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default"


@pytest.fixture(scope="module")
def docs():
    corpora = S.step_corpora()
    S.check_step_conditions(corpora)
    return {"fuzz": corpora, "groups": S.groups(), "bases": S.base_corpus() + S.base_hand_docs()}


# ------------------------------------------------------------------------------------------------------------------- (a) known answers
def test_two_imports_are_not_one_import():
    a = wire.Replica(1)
    a.text_insert("text", 0, "ab"); a.list_insert("list", 0, [1, 2]); a.map_set("map", "k", 1); a.commit()
    v1 = list(a.frontiers)
    a.text_delete("text", 0, 2); a.list_delete("list", 0, 2); a.map_delete("map", "k"); a.commit()
    first, second = a.changes[1]
    assert _merge_ref.Model([first, second]).json() == b'{"map":{}}'            # one import of both never sees the text
    s = _merge_ref.Session([first, second])
    got = [s.step([first]), s.step([second]), s.step([], v1), s.step([]), s.step([], [])]
    assert [g[1] for g in got] == [b'{"list":[1,2],"map":{"k":1},"text":"ab"}', b'{"list":[],"map":{},"text":""}',
                                   b'{"list":[1,2],"map":{"k":1},"text":"ab"}', b'{"list":[],"map":{},"text":""}', b'{"list":[],"map":{},"text":""}']
    assert [g[2] for g in got] == [wire.encode_vv({1: 5}), wire.encode_vv({1: 10}), wire.encode_vv({1: 5}), wire.encode_vv({1: 10}), wire.encode_vv({})]
    d = S.StepDoc("two imports", [first, second], [([S.part([first])], None), ([S.part([second])], None), ([], v1), ([], None), ([], [])])
    assert d.want == got and d.sticky == {wire.root_cid("text", wire.KIND_TEXT), wire.root_cid("list", wire.KIND_LIST)}
    o = _oracle.Session()
    assert [o.step(b, f) for b, f in d.wire_steps()] == got


def test_pending_changes_carry_over_and_resolve():
    a, b = wire.Replica(5), wire.Replica(9)
    a.text_insert("text", 0, "base"); a.commit()
    b.merge_from(a); b.set_visible("text", wire.KIND_TEXT, _merge_ref.view(b, S.TEXT))
    b.text_insert("text", 4, "!"); b.commit()
    s = _merge_ref.Session(a.changes[5] + b.changes[9])
    assert s.step(b.changes[9]) == (0, b"{}", wire.encode_vv({}), 1)
    assert s.step([]) == (0, b"{}", wire.encode_vv({}), 1)
    assert s.step(a.changes[5], [(5, 1)]) == (0, b'{"text":"ba"}', wire.encode_vv({5: 2}), 0)
    assert s.step([]) == (0, b'{"text":"base!"}', wire.encode_vv({5: 4, 9: 1}), 0)


def test_the_layout_rule_is_the_sources():
    """the region of a new peer and the host's sizes, as `Layout` restates them, against the source text"""
    here = os.path.dirname(os.path.abspath(__file__))
    span = open(os.path.join(here, "..", "loro_amd", "csrc", "lm_k_integrate_span.h")).read()
    pipe = open(os.path.join(here, "..", "loro_amd", "csrc", "lm_pipeline.h")).read()
    assert span.count("((ext + ext / 2 + 64 + 31) & ~31u)") == 2 and "d.peer_ext[m.praw0 + lo] <= tk_ecap(tk, rd.pcap)[q]" in span
    assert "uint64_t need = (uint64_t)m.atoms + m.atoms / 2 + 96ull * (m.n_peers + 1) + 8;" in pipe
    assert "uint64_t cap = ((need + need / 2 + 80ull * 8) + 31) & ~31ull;" in pipe
    assert "uint32_t cap = lc + lc / 2 + 8;" in pipe and "uint32_t pcap = P + P / 2 + 2, ccap = C + C / 2 + 4;" in pipe
    assert "uint32_t lc = ok ? m.n_elems / 32 + 2 * m.n_cont + 2 : 0;" in pipe and "uint64_t items = 3ull * m.n_op + 2ull * m.n_nodes * m.n_peers + 64;" in pipe
    assert [S.region(e) for e in (0, 1, 31, 32, 33, 1000)] == [64, 96, 128, 128, 128, 1568]


# ------------------------------------------------------------------------------------------------------------------- (b) the oracle
def test_model_sessions_against_the_oracle(docs):
    n = 0
    for name, ds in list(docs["fuzz"].items()) + [(g[0], g[2]) for g in docs["groups"]] + [("bases", [d.steps for d in docs["bases"]])]:
        for d in ds:
            o = _oracle.Session()
            for k, (blobs, fr) in enumerate(d.wire_steps()):
                got = o.step(blobs, fr)
                assert got == d.want[k], "%s, %s, step %d at %s:\n oracle %r\n model  %r" % (name, d.label, k, d.steps[k][1], got, d.want[k])
                n += 1
            o.close()
    assert n >= 160 * 6


# ------------------------------------------------------------------------------------------------------------------- (c) the harness
def test_resident_documents_need_the_span_kernel(monkeypatch):
    d = S.new_peer_docs("text")[0]
    monkeypatch.setenv("LM_SPAN", "0")
    with Context(_emu.binding()) as c, pytest.raises(RuntimeError, match="span-granular"):
        S.run_group(c, "LM_SPAN=0", [d])


@pytest.mark.parametrize("env", ENVS, ids=ids_of)
def test_fuzz_sessions_in_the_harness(docs, monkeypatch, env):
    """… and the fallback cap: the documents replayed from the empty version at steps >= 1 are no more than the (document, step) pairs
    for which the restated rules say the tracker cannot be used — per corpus and step; those pairs are a quarter of all at most"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pairs = predicted = 0
    for name, ds in docs["fuzz"].items():
        with Context(_emu.binding()) as c:
            seen = S.run_group(c, name, ds, what="kernel %s" % (env or ""))
        per = [S.predicted_fresh(d) for d in ds]
        cap = [sum(x[k] for x in per) for k in range(5)]
        assert seen[0] <= len(ds) and all(s <= m for s, m in zip(seen[1:], cap)), (name, seen, cap)
        pairs += 5 * len(ds); predicted += sum(cap)
    assert predicted * 4 <= pairs, (predicted, pairs)


@pytest.mark.parametrize("env", ENVS, ids=ids_of)
def test_hand_built_groups_in_the_harness(docs, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name, genv, ds, fresh in docs["groups"]:
        for k, v in genv.items():
            monkeypatch.setenv(k, v)
        with Context(_emu.binding()) as c:
            S.run_group(c, name, ds, fresh, what="kernel %s" % (dict(env, **genv) or ""))
            assert "LM_DIR_OPT_MAX" not in genv or c.sizing()[3] >= 1, name
        for k in genv:
            monkeypatch.delenv(k)


# ------------------------------------------------------------------------------------------------------------------- (d) snapshot bases
BASE_ENVS = [{}, {"LM_SNAPSHOT_STATE": "2"}, {"LM_SNAPSHOT_STATE": "2", "LM_PD_STATE_PIECES": "0"}, {"LM_SNAPSHOT_STATE": "0"}, {"LM_SPAN": "0"}, {"LM_PLAIN": "0"}]


def base_counts(bases, env):
    """(state_documents(), redo_documents()) of the batch: the documents rebase_updates_on_state takes, unless the state path is off;
    handed to the history replay: under LM_PD_STATE_PIECES=0 those with more by-position pieces than a document is left with, under
    LM_SPAN=0 every one that deletes base content (the element-granular kernel has no by-position path)"""
    if env.get("LM_SNAPSHOT_STATE") == "0":
        return 0, 0
    taken = [d for d in bases if d.taken]
    redo = sum(d.deletes_base for d in taken) if env.get("LM_SPAN") == "0" else sum(d.many_pieces for d in taken) if env.get("LM_PD_STATE_PIECES") == "0" else 0
    return len(taken), redo


def run_bases(ctx, bases, env, what):
    got = ctx.merge_batch([d.batch for d in bases])
    for d, g in zip(bases, got):
        if g != d.want:
            raise AssertionError("%s %s, %s:\n %s %r\n model  %r\n oracle %r" % (what, env, d.label, what, g, d.want, _oracle.merge(d.batch)))
    counts = (ctx.b.state_documents(ctx.h), ctx.b.redo_documents(ctx.h))
    assert counts == base_counts(bases, env), "%s: state_documents, redo_documents = %r, expected %r" % (env, counts, base_counts(bases, env))


@pytest.mark.parametrize("env", BASE_ENVS, ids=ids_of)
def test_snapshot_bases_as_one_batch(docs, monkeypatch, env):
    bases = docs["bases"]
    assert len(bases) >= 30 and sum(d.deletes_base for d in bases) >= 20 and sum(not d.taken for d in bases) == 1
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Context(_emu.binding()) as c:
        run_bases(c, bases, env, "kernel")


def test_snapshot_bases_as_resident_documents(docs):
    """the snapshot first, then every peer's updates as a step: a resident document stages the snapshot's history, every step continues"""
    n = max(len(d.steps.steps) for d in docs["bases"])
    ds = [d.steps.padded(n) for d in docs["bases"]]
    with Context(_emu.binding()) as c:
        S.run_group(c, "snapshot bases", ds, [len(ds)] + [0] * (n - 1))
