"""Every legal column encoding against the plain model (tests/_column_forms.py), on the CPU: the plain reader against the canonical
writer and the Rust-written blocks, legality of every form, the conditions a corpus must meet, then model = oracle = kernel-logic
harness under the decoder settings of test_emu_parity.py::test_block_decoders_agree and the Map settings of _merge_docs_map, the
byte equality of lm_export, and the zero-length BoolRle runs.

Time, one process on an 8-thread host: the module about 250 s (325 s beside other work) — the documents and their models 40 s (built once per
process, functools.lru_cache), legality and conditions 8 s, the corpus on the harness (488 entries) 10 - 13 s under each of three decoder
settings and a quarter of it 3 s under each of the other six, the hand-built entries 7 - 13 s under each of nine, the Map documents 4 - 15 s
under each of five Map settings (each with and without the second launch), steps and snapshots 3 - 4 s per setting, export 4 s."""
import json, os

import pytest

import _column_forms as F, _emu, _merge_docs_map as M, _oracle
from loro_amd._cabi import Context

FX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures.json")))


def oracle(blobs):
    return _oracle.merge(blobs)


@pytest.fixture(scope="module")
def corpus():
    return F.corpus_entries()


@pytest.fixture(scope="module")
def hand():
    return F.boundary_entries() + F.tail_entries() + F.width_entries()


def legal(entries):
    n = 0
    for d, spec in entries:
        if spec is not None:
            canon, var = d.blocks(), d.blocks(spec)
            assert len(canon) == len(var), d.label
            for v, k in zip(var, canon):
                F.same_values(v, k)
                n += 1
    return n


# ------------------------------------------------------------------------------------------------------------- the reader and the forms
def test_reader_against_the_canonical_writer():
    """every column value the writer was GIVEN comes back from the bytes it wrote (DeltaRle columns: the deltas)"""
    docs, _ = F.fuzz_docs()
    n = 0
    for d in docs[::3] + [F.many_change_doc(65), F.boundary_doc()] + F.dod_docs()[::4]:
        rec = []
        with F.forms(record=rec):
            blobs = d.write(d.reps)
        blocks = [b for blob in blobs for b in F.blocks_of(blob)]
        assert len(blocks) == len(rec)
        for b, given in zip(blocks, rec):
            got = F.read_block(b)["cols"]
            assert sorted(got) == sorted(given)
            for name, vals in given.items():
                assert got[name].values == vals, (d.label, name)
                n += len(vals)
    assert n > 10000


def test_reader_against_rust_written_blocks():
    """the change blocks of the reference's own update blobs: every column is used up exactly, the counts agree with one another
    (read_block raises otherwise: op columns of equal length, the atom lengths sum to the block's counter span, the dependency counts
    sum to the dependency columns' lengths), and the segmentation the Rust writer chose is one the forms cover"""
    n_blocks = n_rows = 0
    for name, hexed in FX["blobs"].items():
        blob = bytes.fromhex(hexed)
        if blob[20:22] != b"\x00\x04":
            continue
        for b in F.blocks_of(blob):
            blk = F.read_block(b)
            c = blk["cols"]
            assert len(c["dep_self"].values) == len(c["dep_count"].values) == len(c["timestamp"].values) == blk["head"][4]
            assert len(c["lamport"].values) == blk["head"][4] - 1 and len(c["dep_peer"].values) == len(c["dep_ctr"].values) == sum(c["dep_count"].values)
            assert all(p < len(blk["peers"]) for p in c["dep_peer"].values)
            if "del_peer" in c:
                assert all(0 <= p < len(blk["peers"]) for p in c["del_peer"].sums)
            n_blocks += 1
            n_rows += len(c["len"].values)
    assert n_blocks >= 5 and n_rows >= 50, (n_blocks, n_rows)


def test_forms_are_restored_and_selected_per_column():
    from loro_amd import wire
    orig = (wire._any_rle, wire.enc_delta_of_delta, wire.enc_bool_rle)
    with pytest.raises(ZeroDivisionError):
        with F.forms(any_rle="run1"):
            assert wire._any_rle is not orig[0]
            1 / 0
    assert (wire._any_rle, wire.enc_delta_of_delta, wire.enc_bool_rle) == orig
    d = F.many_change_doc(17)
    canon = F.read_block(d.blocks()[0])["cols"]
    got = F.read_block(d.blocks({"any_rle": {"dep_count": "run1"}, "dod": {"lamport": "widest"}})[0])["cols"]
    assert all(s[:2] == ("run", 1) for s in got["dep_count"].segs) and set(got["lamport"].segs) == {5}
    for name in ("dep_peer", "cidx", "prop", "vtype", "len", "dep_ctr", "timestamp"):
        assert [s[:2] for s in got[name].segs] == [s[:2] for s in canon[name].segs] if name in F.ANY_COLS else got[name].segs == canon[name].segs, name


def test_every_form_is_legal_and_the_corpus_meets_the_conditions(corpus, hand):
    assert legal(corpus) >= 1000 and legal(hand) >= 100
    counts = F.counts_of(corpus)
    print("\n%d blocks\n%s" % (counts.blocks, counts.table()))
    F.check_conditions(counts)


def test_the_last_bytes_of_a_column():
    """the prop column's last value starts 1, 2 and 3 bytes before the column's end, its last segment head 2 and 3 bytes before
    it (a head is followed by a value: 1 cannot be), and the byte BEHIND the column — the value-type column's length prefix — has
    its top bit set: a reader that looks past its end reads another number"""
    value_at, head_at = set(), set()
    for d, spec in F.tail_entries():
        if spec is None:
            continue
        raw = d.blocks(spec)[0]
        col = F.read_block(raw)["cols"]["prop"]
        assert raw[col.end] & 0x80, (d.label, spec)
        value_at.add(col.end - col.segs[-1][3][-1])
        head_at.add(col.end - col.segs[-1][2])
    assert value_at >= {1, 2, 3} and head_at >= {2, 3}, (value_at, head_at)


def test_segment_ends_at_the_row_chunk_and_the_row_store():
    d = F.boundary_doc()
    for col in F.ROW_COLS:
        for first in ("run", "lit"):
            segs = F.read_block(d.blocks({"any_rle": {col: ("cut", F.BOUNDARY_ROWS, first)}})[0])["cols"][col].segs
            ends, row = set(), 0
            for s in segs:
                row += s[1]
                ends.add(row)
            assert ends >= set(F.BOUNDARY_ROWS), (col, first)
            kinds = {s[0] for s in segs}
            assert kinds == {"run", "lit"}, (col, first)


# --------------------------------------------------------------------------------------------------------- model = oracle = harness
def test_model_against_oracle(corpus, hand):
    entries = corpus + hand
    got = _oracle.merge_batch([d.blobs(spec) for d, spec in entries], threads=8)
    for (d, spec), g in zip(entries, got):
        assert g == d.expect(), (d.label, spec, g[:3], d.expect()[:3])


def under(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS[:3], ids=[s[0] for s in F.DECODER_SETTINGS[:3]])
def test_corpus_against_harness(corpus, monkeypatch, setting):
    under(monkeypatch, setting[1])
    with Context(_emu.binding()) as c:
        assert F.run_entries(c, corpus, setting[0], oracle) == len(corpus)


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS[3:], ids=[s[0] for s in F.DECODER_SETTINGS[3:]])
def test_every_fourth_corpus_entry_against_harness(corpus, monkeypatch, setting):
    """the six other decoder settings take a quarter of the corpus here (whole documents: a canonical twin with its variants) — ten
    seconds per setting for all of it was the price; the device module runs the whole corpus under all nine"""
    under(monkeypatch, setting[1])
    by_doc = {}
    for d, spec in corpus:
        by_doc.setdefault(id(d), []).append((d, spec))
    sub = [e for es in list(by_doc.values())[::4] for e in es]
    with Context(_emu.binding()) as c:
        assert F.run_entries(c, sub, setting[0], oracle) == len(sub) >= 100


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS[:3], ids=[s[0] for s in F.DECODER_SETTINGS[:3]])
def test_documents_in_steps(monkeypatch, setting):
    """resident documents (stage + import_more, three steps): results after every step and resident_fresh() equal to the canonical run's"""
    under(monkeypatch, setting[1])
    with Context(_emu.binding()) as c:
        assert F.check_steps(c, setting[0]) >= 90


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS[:4], ids=[s[0] for s in F.DECODER_SETTINGS[:4]])
def test_documents_inside_a_snapshot(monkeypatch, setting):
    """the same blocks in the ChangeStore of a FastSnapshot whose state section holds placeholders: the history path"""
    under(monkeypatch, setting[1])
    entries = F.path_entries(", a snapshot", F.as_snapshot)
    with Context(_emu.binding()) as c:
        assert F.run_snapshots(c, entries, setting[0]) == len(entries) >= 90


def test_documents_beyond_the_limits():
    with Context(_emu.binding()) as c:
        F.check_limits(c)
        F.check_message_sum(c)


@pytest.mark.parametrize("setting", F.DECODER_SETTINGS, ids=[s[0] for s in F.DECODER_SETTINGS])
def test_hand_built_documents_against_harness(hand, monkeypatch, setting):
    """segment ends at rows 7-9 / 63-65, the last bytes of a column, run counts of 63 / 64 and 8,191 / 8,192, the DeltaOfDelta edges
    and the many-change blocks, under every decoder setting"""
    under(monkeypatch, setting[1])
    entries = hand + F.dod_entries() + F.many_change_entries()
    with Context(_emu.binding()) as c:
        assert F.run_entries(c, entries, setting[0], oracle) == len(entries)


@pytest.mark.parametrize("setting", M.SETTINGS, ids=[s[0] for s in M.SETTINGS])
def test_map_documents_keep_their_path(monkeypatch, setting):
    """Map documents (the fuzz Map sessions, key tables beyond the default slot, the 8,192-row runs) under the Map settings, with
    LM_DEC_SLOT_BIG both ways: a form must not move a document off the fused path — the batch of variants shows the
    fused_documents / redo_documents that _column_forms.MAP_PATHS states for the setting, as literals"""
    name, env, fused_on, ht_opt = setting
    for big in ({}, {"LM_DEC_SLOT_BIG": "0"}):
        under(monkeypatch, dict(env, **big))
        with Context(_emu.binding()) as c:
            assert F.check_map_paths(c, name, oracle) == 68


def test_export_gives_back_the_canonical_bytes(corpus, hand):
    """lm_export from the empty version: a variant document exports, byte for byte, what its canonical twin exports"""
    entries = [e for e in corpus + hand if e[1] is not None][::5]
    with Context(_emu.binding()) as c:
        c.stage([d.blobs(spec) for d, spec in entries]); c.run()
        assert all(g[0] == 0 for g in c.fetch())
        var = [c.export(i) for i in range(len(entries))]
        c.stage([d.blobs() for d, _ in entries]); c.run()
        canon = [c.export(i) for i in range(len(entries))]
    for (d, spec), a, b in zip(entries, var, canon):
        assert a == b, (d.label, spec)
    assert len(entries) >= 80


# ----------------------------------------------------------------------------------------------------------------- the BoolRle finding
def test_zero_length_bool_runs():
    """dep_on_self with F0 / T0 pairs in front of the real runs and between two real runs.  One pair (at most three zero-length runs in
    a row) is read by kernels and oracle alike and changes nothing; two, three and eight pairs are REFUSED by both with the same
    status, LM_DECODE_ERROR (1): bool_next reads at most four run lengths for one value, oracle/lo_codec.hpp says the same since.
    The grammar text allows a zero FIRST run only; the decision is in NEXT.md."""
    for d in F.bool_docs():
        canon = F.read_block(d.blocks()[0])["cols"]["dep_self"]
        for form in F.BOOL_ACCEPTED + F.BOOL_REFUSED:
            col = F.read_block(d.blocks({"bool_rle": form})[0])["cols"]["dep_self"]
            assert col.values == canon.values and len(col.segs) == len(canon.segs) + 2 * form[1], (d.label, form)      # legal under the loose reading
        with Context(_emu.binding()) as c:
            F.run_entries(c, [(d, None)] + [(d, {"bool_rle": f}) for f in F.BOOL_ACCEPTED], "zero runs", oracle)
            for f in F.BOOL_REFUSED:
                blobs = d.blobs({"bool_rle": f})
                got, ora = c.merge_batch([blobs, d.blobs()]), _oracle.merge(blobs)
                assert got[0][0] == ora[0] == 1 and got[0][1] == ora[1] == b"", (d.label, f, got[0][:2], ora[:2])
                assert got[1] == d.model.result()                      # the neighbour in the batch is not disturbed
        for f in F.BOOL_ACCEPTED:
            assert _oracle.merge(d.blobs({"bool_rle": f})) == d.model.result()
