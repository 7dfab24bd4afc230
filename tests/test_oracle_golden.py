"""The CPU oracle pinned against the reference's own golden vectors and known-answer tests."""
import gzip, json, os
import pytest

import _oracle, _cases
from loro_amd import wire

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "reference_fixtures.json")))
BLOB = {k: bytes.fromhex(v) for k, v in FX["blobs"].items()}


def deep(blobs):
    st, js, vv, pend = _oracle.merge(blobs)
    return st, json.loads(js), vv, pend


def test_xxh32_matches_envelope_of_rust_written_blob():
    b = BLOB["updates.blob"]
    assert b[:4] == b"loro" and b[20:22] == b"\x00\x04"
    # checksum of the Rust-encoded fixture
    assert int.from_bytes(b[16:20], "little") == 0x030E3A92
    assert _oracle.xxh32(b[20:]) == 0x030E3A92
    assert wire.xxh32(b[20:]) == 0x030E3A92


def test_fugue_fixture_both_import_orders():
    # crates/loro/tests/loro_js_interop.rs:114-126
    for order in (("fugue-left.ts.blob", "fugue-right.ts.blob"), ("fugue-right.ts.blob", "fugue-left.ts.blob")):
        st, v, _, pend = deep([BLOB[n] for n in order])
        assert st == 0 and pend == 0 and v == {"text": "Hello World!"}


def test_concurrent_fixture_both_import_orders():
    # crates/loro/tests/loro_js_interop.rs:97-112 ; Counter/mergeable keys are outside the hot-path scope
    want = FX["json"]["concurrent.expected.json"]
    for order in (("concurrent-base.ts.blob", "concurrent-left.ts.blob", "concurrent-right.ts.blob"),
                  ("concurrent-base.ts.blob", "concurrent-right.ts.blob", "concurrent-left.ts.blob")):
        st, v, _, _ = deep([BLOB[n] for n in order])
        assert st == 4  # LM_UNSUPPORTED flag: a Counter container is present
        for k in ("list", "text", "map"):
            assert v[k] == want[k]


@pytest.mark.parametrize("name", ["updates.blob", "updates.ts.blob"])
def test_rust_updates_fixture_matches_deep_json(name):
    # crates/loro/tests/loro_js_interop.rs:42-63 (Rust- and TS-encoded bytes of the same history)
    want = FX["json"]["snapshot.deep.json"]
    st, v, vv, pend = deep([BLOB[name]])
    assert pend == 0
    # snapshot.deep.json is the deep value of a SNAPSHOT import (its state section carries every container state of the
    # exporting document, `imports_typescript_reencoded_snapshot`); for the updates blobs the reference only asserts
    # Rust-bytes == TS-bytes.  "list" and "text" end empty in this history, so an UPDATES import creates no state for
    # them (diff_calc.rs:299, state.rs:1365): absent here, empty there.
    assert v.get("list", []) == want["list"] == [] and v.get("text", "") == want["text"] == ""
    for k, x in want["map"].items():
        if k == "child_tree":  # Tree children: out of scope (the MovableList child is compared: SURVEY.md §8f N4)
            continue
        assert v["map"][k] == x, k
    # version vector of the fixture: 3 peers, 40 ops (meta.json) — decoded from the postcard map
    assert vv[0] == 3


def test_runtime_fixture_supported_keys():
    want = FX["json"]["runtime.expected.json"]
    st, v, _, _ = deep([BLOB["runtime-updates.ts.blob"]])
    assert v["list"] == want["list"] and v["text"] == want["text"]
    for k in ("answer", "child", "nested"):
        assert v["map"][k] == want["map"][k]


# ---- crates/loro-internal/tests/fugue.rs:5-90 expressed as edit scripts through the FastUpdates writer
def _merge_replicas(*reps):
    blobs = [r.export() for r in reps]
    out = set()
    import itertools
    for perm in itertools.permutations(blobs):
        st, js, _, pend = _oracle.merge(list(perm))
        assert st == 0 and pend == 0
        out.add(js)
    assert len(out) == 1, "import order changed the result"
    return json.loads(out.pop())


def test_fugue_forward_interleaving():
    a = wire.Replica(0); a.text_insert("text", 0, "Hello"); a.commit()
    b = wire.Replica(1); b.text_insert("text", 0, " World!"); b.commit()
    assert _merge_replicas(a, b) == {"text": "Hello World!"}


def test_fugue_backward_interleaving():
    a = wire.Replica(0)
    for ch in "olleH":
        a.text_insert("text", 0, ch)
    a.commit()
    b = wire.Replica(1)
    for ch in "!dlroW ":
        b.text_insert("text", 0, ch)
    b.commit()
    assert _merge_replicas(a, b) == {"text": "Hello World!"}


def test_fugue_forward_backward():
    a = wire.Replica(0); a.text_insert("text", 0, "ll"); a.text_insert("text", 0, "He"); a.text_insert("text", 4, "o"); a.commit()
    b = wire.Replica(1); b.text_insert("text", 0, " !"); b.text_insert("text", 1, "W")
    for ch in "dlro":
        b.text_insert("text", 2, ch)
    b.commit()
    assert _merge_replicas(a, b) == {"text": "Hello World!"}


def test_fugue_yjs_interleave_anomaly():
    a, b, c = wire.Replica(0), wire.Replica(1), wire.Replica(2)
    c.text_insert("text", 0, "2"); c.commit()
    a.merge_from(c); a.set_visible("text", wire.KIND_TEXT, list(c.seq[wire.root_cid("text", wire.KIND_TEXT)]))
    a.text_insert("text", 0, "1"); a.commit()
    b.text_insert("text", 0, "b"); b.commit()
    own_a = wire.Replica(0); own_a.changes = {0: a.changes[0]}
    assert _merge_replicas(own_a, b, c) == {"text": "b12"}


def test_map_lww_peer_tiebreak_and_delete():
    # equal lamports: larger peer wins (delta/map_delta.rs:26-32); a delete competes like a write (map_state.rs:438-449)
    a = wire.Replica(5); a.map_set("map", "k", "from5"); a.map_set("map", "gone", 1); a.commit()
    b = wire.Replica(9); b.map_set("map", "k", "from9"); b.map_delete("map", "gone"); b.commit()
    assert _merge_replicas(a, b) == {"map": {"k": "from9"}}


def test_pending_change_is_parked_then_applied():
    a = wire.Replica(1); a.text_insert("text", 0, "ab"); a.commit()
    first = a.export()
    a.text_insert("text", 2, "cd"); a.commit()
    second = a.export({1: 2})
    st, js, vv, pend = _oracle.merge([second])
    assert (st, js, pend) == (0, b"{}", 2) and vv == wire.encode_vv({})
    st, js, vv, pend = _oracle.merge([second, first])
    assert (st, js, pend) == (0, b'{"text":"abcd"}', 0) and vv == wire.encode_vv({1: 4})


def test_errors_mirror_loro_error_kinds():
    a = wire.Replica(1); a.text_insert("text", 0, "ab"); a.commit()
    good = a.export()
    bad_sum = bytearray(good); bad_sum[-1] ^= 1
    assert _oracle.merge([bytes(bad_sum)])[0] == 2          # DecodeChecksumMismatchError
    assert _oracle.merge([b"lor0" + good[4:]])[0] == 1       # DecodeError: bad magic
    assert _oracle.merge([good[:10]])[0] == 1                # DecodeError: too short


REF_TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "automerge-paper.json.gz")   # the reference's crates/loro-internal/benches/automerge-paper.json.gz, stored as it is


def test_automerge_paper_trace_end_content():
    """benches/automerge-paper.json.gz: applying all 259,778 patches must give `endContent`."""
    d = json.load(gzip.open(REF_TRACE))
    r = wire.Replica(1)
    k = 0
    for tx in d["txns"]:
        for pos, dl, s in tx["patches"]:
            if dl:
                r.text_delete("text", pos, dl)
            if s:
                r.text_insert("text", pos, s)
            k += 1
            if k % 1000 == 0:
                r.commit()
    r.commit()
    st, js, vv, pend = _oracle.merge([r.export()])
    assert st == 0 and pend == 0
    assert json.loads(js)["text"] == d["endContent"]


# ---- checkout (time travel): known answers of crates/loro-internal/tests/test.rs
def _at(blobs, ids):
    return _oracle.merge(blobs, frontiers=wire.encode_frontiers(ids))


def test_text_checkout_known_answers():
    """test.rs:518-585 `test_text_checkout`: state of the text after each op counter."""
    r = wire.Replica(1)
    r.text_insert("text", 0, "你界")
    r.text_insert("text", 1, "好世")
    r.commit()
    blobs = [r.export()]
    for ctr, want in enumerate(["你", "你界", "你好界", "你好世界"]):
        st, js, vv, _ = _at(blobs, [(1, ctr)])
        assert st == 0 and json.loads(js) == {"text": want}
        assert vv == wire.encode_vv({1: ctr + 1})
    r.text_delete("text", 3, 1)
    r.text_delete("text", 2, 1)
    r.commit()
    blobs = [r.export()]
    assert json.loads(_oracle.merge(blobs)[1]) == {"text": "你好"}
    for ctr, want in [(3, "你好世界"), (4, "你好世"), (5, "你好"), (0, "你"), (1, "你界"), (2, "你好界")]:
        assert json.loads(_at(blobs, [(1, ctr)])[1]) == {"text": want}
    # the empty version keeps the root container the state store knows, with an empty value
    st, js, vv, _ = _at(blobs, [])
    assert (st, js, vv) == (0, b'{"text":""}', wire.encode_vv({}))
    # FrontiersNotFound (loro.rs:1699-1701)
    assert _at(blobs, [(1, 6)])[0] == 6 and _at(blobs, [(2, 0)])[0] == 6


def test_map_checkout_known_answers():
    """test.rs:587-603 `map_checkout` and :659-693 `map_concurrent_checkout`."""
    r = wire.Replica(5)
    r.map_set("meta", "key", 0); r.commit()
    r.map_set("meta", "key", 1); r.commit()
    blobs = [r.export()]
    assert json.loads(_at(blobs, [(5, 0)])[1]) == {"meta": {"key": 0}}
    assert json.loads(_at(blobs, [])[1]) == {"meta": {}}
    assert json.loads(_at(blobs, [(5, 1)])[1]) == {"meta": {"key": 1}}
    a, b = wire.Replica(1), wire.Replica(2)
    a.map_set("meta", "key", 0); a.commit()
    va = list(a.frontiers)
    b.map_set("meta", "s", 1); b.commit()
    vb0 = list(b.frontiers)
    b.map_set("meta", "key", 1); b.commit()
    vb1 = list(b.frontiers)
    a.merge_from(b)
    a.map_set("meta", "key", 2); a.commit()
    vm = list(a.frontiers)
    blobs = [a.export()]
    for v, want in [(va, {"key": 0}), (vb0, {"s": 1}), (vb1, {"s": 1, "key": 1}), (vm, {"s": 1, "key": 2})]:
        assert json.loads(_at(blobs, v)[1]) == {"meta": want}
    # a frontier with both heads before the merge: both branches, LWW between key=0 (lamport 0, peer 1) and key=1 (lamport 1)
    assert json.loads(_at(blobs, va + vb1)[1]) == {"meta": {"s": 1, "key": 1}}


def test_checkout_equals_import_of_the_prefix():
    """Checking out version V of the full history equals importing only the updates up to V (CRDT state is a
    function of the op set): random concurrent sessions, every intermediate frontier of one replica."""
    import _fuzz
    n = 0
    for s in range(8):
        snaps = []
        reps = _fuzz.random_session(900 + s, n_peers=3, n_steps=60, kinds=("text", "list", "map"), styles=True, snapshots=snaps)
        full = _fuzz.blobs_of(reps)
        for fr, blob in snaps:
            got = _oracle.merge(full, frontiers=wire.encode_frontiers(fr))
            want = _oracle.merge([blob])
            assert got[0] == want[0] == 0
            # same value for every container the prefix knows; containers created later render empty
            gj, wj = json.loads(got[1]), json.loads(want[1])
            for k, v in gj.items():
                assert wj.get(k, type(v)()) == v, (s, fr, k)
            assert got[2] == want[2], (s, fr)
            n += 1
    assert n > 20


def _two_peer_delete_doc(backspace):
    """peer 1 types 10 chars; peer 2 (having seen them) deletes all ten — forward in one op, or by ten backspaces
    that the writer RLE-merges into one reversed DeleteSeq (signed_len = -10)."""
    a, b = wire.Replica(1), wire.Replica(2)
    a.text_insert("text", 0, "abcdefghij"); a.commit()
    b.merge_from(a)
    b.set_visible("text", wire.KIND_TEXT, _oracle.visible_ids([a.export()], "text", wire.KIND_TEXT))
    if backspace:
        for i in range(9, -1, -1):
            b.text_delete("text", i, 1)
    else:
        b.text_delete("text", 0, 10)
    b.commit()
    ops = b.changes[2][0].ops
    assert len(ops) == 1 and ops[0].signed_len == (-10 if backspace else 10)
    return [b.export()]


def test_tracker_known_answers_through_checkout():
    """container/richtext/tracker.rs:734-773 — `test_retreat_and_forward_delete` (reversed delete: checking out
    2=>5 of 10 leaves 5 elements, 2=>0 all 10, 2=>10 none) and `test_checkout_in_doc_with_del_span` (forward delete,
    2=>4: the first 4 elements inactive, the other 6 active), restated as documents + checkouts."""
    rev = _two_peer_delete_doc(True)
    assert json.loads(_at(rev, [(2, 4)])[1]) == {"text": "abcde"}
    assert json.loads(_at(rev, [(1, 9)])[1]) == {"text": "abcdefghij"}
    assert json.loads(_at(rev, [(2, 9)])[1]) == {}   # nothing visible at the latest version nor here: the root never got a state (diff_calc.rs:299)
    fwd = _two_peer_delete_doc(False)
    assert json.loads(_at(fwd, [(2, 3)])[1]) == {"text": "efghij"}
    assert _at(fwd, [(2, 3)])[2] == wire.encode_vv({1: 10, 2: 4})
    # tracker.rs:720-732 `test_len`: two peers insert 2 elements each at position 0 from the empty version
    a, b = wire.Replica(1), wire.Replica(2)
    a.text_insert("text", 0, "ab"); a.commit()
    b.text_insert("text", 0, "cd"); b.commit()
    both = [a.export(), b.export()]
    assert len(json.loads(_oracle.merge(both)[1])["text"]) == 4
    assert json.loads(_at(both, [(1, 1)])[1]) == {"text": "ab"}
    assert json.loads(_at(both, [])[1]) == {"text": ""}


def test_oracle_rejects_damaged_documents_without_crashing():
    """The oracle is the checker, so it must survive anything the parity tests feed it: a damaged document (byte flips,
    truncation, splices; checksum re-fitted) either decodes or raises a LoroError-kind status — never an out-of-bounds
    read.  tests/golden/damaged_placeholder_span.json is the document that used to crash it (a delete of ids no insert
    produced left a visible span without content); inserts whose content does not match their `len` column entry are
    rejected at decode (docs/encoding.md §10.6, lo_codec.hpp)."""
    import json, os
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "damaged_placeholder_span.json")))
    st = _oracle.merge_batch([[bytes.fromhex(h) for h in fx["blobs_hex"]]], threads=1)[0][0]
    assert st == 3          # LM_DATA_CORRUPTION
    for seed in (12, 21, 22):
        docs = _cases.corrupted_docs(400, seed=seed)
        res = _oracle.merge_batch(docs, threads=8)
        assert {r[0] for r in res} <= {0, 1, 2, 3, 4}
        assert any(r[0] == 0 for r in res) and any(r[0] != 0 for r in res)


# ---- the STATE section of the snapshot fixtures, read for its values (oracle/lo_state.hpp; groundwork for SURVEY §8f N3)
@pytest.mark.parametrize("name", ["snapshot.blob", "snapshot.ts.blob", "runtime-snapshot.ts.blob"])
def test_snapshot_state_section_holds_the_value_its_history_gives(name):
    """docs/encoding-container-states.md as read by lo_state.hpp (ContainerWrapper, postcard LoroValue / ContainerID, Map / List /
    Text / MovableList visible values) against Rust- and TS-written snapshots: the value rendered from the state section ALONE is,
    byte for byte, the value the checker gets by replaying the snapshot's history — and the value the reference expects"""
    st, js = _oracle.snapshot_state(BLOB[name])
    hist = _oracle.merge_batch([[BLOB[name]]])[0]
    assert (st, js) == (hist[0], hist[1])
    v = json.loads(js)
    want = FX["json"]["snapshot.deep.json" if name.startswith("snapshot") else "runtime.expected.json"]
    for k, x in want.items():
        if k in ("tree", "counter"):          # out of the device scope: rendered null, status LM_UNSUPPORTED
            assert v[k] is None and st == 4
            continue
        if isinstance(x, dict):
            for kk, xx in x.items():
                if kk in ("child_tree", "mergeable"):   # Tree child / mergeable-container markers (binary activation values)
                    continue
                assert v[k][kk] == xx, (k, kk)
        else:
            assert v[k] == x, k


def test_shallow_snapshot_state_at_its_latest_version_and_at_its_root():
    # crates/loro/tests/loro_js_interop.rs:129-147: get_deep_value() after the import, and after checkout(shallow_since_frontiers)
    assert _oracle.snapshot_state(BLOB["shallow.ts.blob"]) == (0, b'{"text":"0123456789"}')
    assert _oracle.snapshot_state(BLOB["shallow.ts.blob"], root_only=True) == (0, b'{"text":"01234"}')
    # (the history path cannot render it: the ops below the shallow root are gone — LM_UNSUPPORTED there, oracle and device)
    assert _oracle.merge_batch([[BLOB["shallow.ts.blob"]]])[0][0] == 4


def test_the_state_writer_of_the_test_generators_round_trips_through_the_pinned_reader():
    """oracle/lo_state_write.hpp (the generator behind tests/test_emu_snapshot.py real_snapshot) against lo_state.hpp, the reader the
    tests above pin on the Rust- and TS-written fixtures: write the state of a history, read it back, get the history's value —
    on the fixtures' own histories and on generated sessions (nested children, MovableLists, styled text)"""
    import _fuzz
    from loro_amd import wire
    for name in ("updates.blob", "runtime-updates.ts.blob"):
        st, ents = _oracle.state_entries([BLOB[name]])
        hist = _oracle.merge_batch([[BLOB[name]]])[0]
        snap = wire.encode_snapshot([], [], {}, [], state=ents)
        assert st == hist[0] and _oracle.snapshot_state(snap) == (hist[0], hist[1])
    for seed in range(12):
        reps = [_fuzz.movable_session(seed, n_peers=3, n_steps=60, nested=True), _fuzz.nested_session(seed, n_peers=3, n_steps=80),
                _fuzz.random_session(seed, n_peers=3, n_steps=80, kinds=("text", "list", "map"), styles=True)][seed % 3]
        blobs = _fuzz.blobs_of(reps)
        st, ents = _oracle.state_entries(blobs)
        hist = _oracle.merge(blobs)
        assert st == hist[0] == 0 and _oracle.snapshot_state(wire.encode_snapshot([], [], {}, [], state=ents)) == (0, hist[1])
