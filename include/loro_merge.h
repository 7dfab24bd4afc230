/* loro_merge.h — C ABI of the MI355X batched CRDT merge engine.
 *
 * Drop-in boundary for Loro's import → diff_calc → state path.  The reference has no FFI on this path
 * (SURVEY.md §8b); the boundary therefore sits at the byte interface the Rust host already owns:
 *
 *   input   exactly what `LoroDoc::export(ExportMode::Updates{..})` (or ExportMode::Snapshot, see "Limits") produces and
 *           `LoroDoc::import()` consumes
 *           (crates/loro/src/lib.rs:710,1306; crates/loro-internal/src/encoding.rs:334-373,399-405;
 *           docs/encoding.md §2,§6-10).  The blobs of one document are imported in order, like
 *           `LoroDoc::import_batch` (crates/loro-internal/src/loro.rs:1432-1523), into an empty document.
 *   output  what `doc.get_deep_value().to_json_value()` (crates/loro/src/lib.rs:937,
 *           crates/loro-internal/src/state.rs:1294-1329) and `doc.oplog_vv().encode()`
 *           (crates/loro/src/lib.rs:887, crates/loro-internal/src/version.rs:962-964) produce:
 *           canonical JSON (UTF-8, object keys sorted bytewise, no whitespace) and a postcard map
 *           peer→exclusive counter with entries sorted by peer.
 *
 * Errors are per document and mirror LoroError (crates/loro-common/src/error.rs): a bad document never
 * fails the batch (reference import is per-document atomic, loro.rs:780-838).  Changes whose dependencies
 * are missing are not errors: they are reported as pending (ImportStatus.pending, encoding.rs:227-231) and
 * excluded from state and version vector.
 *
 * Threading: a context is single-caller; several contexts may be used concurrently.
 * Ownership: inputs are borrowed for the duration of the call; outputs belong to the context and stay
 * valid until the next lm_merge_batch / lm_run / lm_destroy on it.
 */
#ifndef LORO_MERGE_H
#define LORO_MERGE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
  LM_OK = 0,
  LM_DECODE_ERROR = 1,       /* LoroError::DecodeError */
  LM_CHECKSUM_MISMATCH = 2,  /* LoroError::DecodeChecksumMismatchError */
  LM_DATA_CORRUPTION = 3,    /* LoroError::DecodeDataCorruptionError */
  LM_UNSUPPORTED = 4,        /* outside the device path's scope — see "Limits" below */
  LM_INTERNAL = 5,
  LM_FRONTIERS_NOT_FOUND = 6 /* LoroError::FrontiersNotFound: a checkout id the imported history does not hold */
};

/* Limits of the device path.  A document beyond one of them is reported LM_UNSUPPORTED — never a guessed value — and
 * does not disturb the other documents of the batch (tests: `documented_limits_are_reported_not_guessed`, emu + GPU):
 *   - container kinds: Map, List, Text, MovableList (root or child; MovableList: insert / delete / move / set, per-element
 *     last-writer-wins of position and value — diff_calc.rs:1669-1993, history_cache.rs:754-1003).  A document that also
 *     holds Tree / Counter containers is rendered with those as null and reported LM_UNSUPPORTED *together with* its JSON
 *     and VV;
 *   - blobs: EncodeMode::FastUpdates (mode 4) and FastSnapshot (mode 3).  A snapshot is ingested on the host in front of
 *     the device path: its history from the ChangeStore section (replayed like updates, fast_snapshot.rs:326-344), the set
 *     of root containers from the keys of its state section (an empty document initialises its state store from that
 *     section, fast_snapshot.rs:168-258, so a root in which nothing is visible is still part of the value).  The first
 *     snapshot among a document's blobs plays that role (import_batch imports snapshots first).  A document that is ONE
 *     snapshot rendered at its latest version is staged from the state section's VALUES instead (lm_state_documents below):
 *     no history is uploaded, decoded or replayed.  Shallow snapshots (history trimmed below a shallow root) are rendered
 *     that way at their latest version and at their shallow root; at any other version, next to other blobs, under
 *     lm_import or lm_richtext they are LM_UNSUPPORTED;
 *   - per document: <= 255 peers, <= 256 containers of which <= 64 roots, container nesting <= 16, counters < 2^24 per
 *     peer (element ids are packed peer:8 | counter:24), < 2^24 Map / MovableList move+set op rows, <= 18,000 tracker leaves per sequence
 *     replay (~190k op runs; the 1M-op documents of BASELINE configs[4] use ~1,200), JSON < 4 GiB, a blob < 4 GiB;
 *   - two root containers with the same name but different kinds; a StyleEnd op that does not directly follow its
 *     StyleStart (every writer emits them as a pair).  */
typedef struct lm_ctx lm_ctx;

typedef struct lm_doc_in {
  const uint8_t* const* blobs; /* n_blobs update blobs (EncodeMode::FastUpdates), imported in order */
  const size_t* blob_lens;
  size_t n_blobs;
  /* Optional checkout (LoroDoc::checkout, crates/loro-internal/src/loro.rs:1625-1760): render the state at
   * these frontiers instead of the latest version.  Bytes = Frontiers::encode() (version/frontiers.rs:219-223:
   * postcard Vec<ID>, sorted).  NULL = latest.  The one-byte encoding 00 is the empty version.  With a checkout
   * the vv output is the version of the rendered state (state_vv), not oplog_vv.  The batch entry replays the version's causal
   * closure only (same bytes as import + checkout on every healthy document); LM_CHECKOUT_FULL=1 in the environment makes it import
   * the whole history first, as the reference does — a document damaged OUTSIDE the rendered version then fails like there. */
  const uint8_t* checkout_frontiers;
  size_t checkout_len;
} lm_doc_in;

typedef struct lm_doc_out {
  int32_t status;       /* LM_* */
  const uint8_t* json;  /* canonical deep-value JSON (not NUL terminated) */
  size_t json_len;
  const uint8_t* vv;    /* postcard VersionVector, entries sorted by peer */
  size_t vv_len;
  uint64_t pending_ops; /* atoms parked because a dependency is missing */
} lm_doc_out;

/* Create a context on HIP device `device` (>= 0).  Returns NULL when no usable MI355X-class device or the
 * HIP runtime is missing — there is no CPU fallback. */
lm_ctx* lm_create(int device);
void lm_destroy(lm_ctx* ctx);
const char* lm_last_error(lm_ctx* ctx);

/* One-shot: stage + run + fetch.  Returns 0 on success (per-document results in outs[i].status). */
int lm_merge_batch(lm_ctx* ctx, const lm_doc_in* docs, size_t n_docs, lm_doc_out* outs);

/* Split form, for callers that keep batches resident in HBM (and for benchmarking the device path):
 * lm_stage packs the blobs and uploads them, lm_run executes the device pipeline on the staged batch
 * (may be repeated), lm_fetch copies the rendered states back and fills outs[0..n_docs). */
int lm_stage(lm_ctx* ctx, const lm_doc_in* docs, size_t n_docs);
int lm_run(lm_ctx* ctx);

/* Direct staging (round 6).  lm_stage copies the blobs host -> pinned staging buffer -> HBM; the first hop (a gather by a few host
 * threads) is what bounds a server that feeds the engine from pageable memory (~38 GB/s on the development box).  A host that
 * receives its blobs INTO memory obtained from lm_host_alloc (pinned; release with lm_host_free) skips it: when every blob of a
 * batch lies inside one such region — each at a 16-byte aligned address, in the order they are staged (document by document, blob
 * by blob), without overlap, and packed reasonably densely (the span from the first blob to the end of the last is copied whole:
 * it must not exceed twice the blobs' bytes + 1 MiB) — lm_stage hands that span to the copy engine as it is and touches no byte
 * of it.  The bytes between blobs are never interpreted.  The region must stay valid and unchanged until the NEXT lm_stage of the
 * context (documents that are replayed — lm_redo_documents, lm_import after a state-staged batch — are read from it again).
 * Anything else (a blob outside the region, unaligned, out of order; a snapshot, which is reframed on the host) takes the gather
 * as before.  lm_staged_direct: 1 when the batch staged last took this path.  LM_STAGE_DIRECT=0 switches it off. */
void* lm_host_alloc(size_t bytes);
void lm_host_free(void* p);
int lm_staged_direct(lm_ctx* ctx);
int lm_fetch(lm_ctx* ctx, lm_doc_out* outs);
/* Asynchronous lm_run: lm_run_async returns at once, lm_wait blocks until that run is finished (0 = ok).  Between the
 * two calls only other contexts may be used.  Two contexts in flight overlap one batch's decode stages with the other's
 * integrate kernels (double buffering). */
int lm_run_async(lm_ctx* ctx);
int lm_wait(lm_ctx* ctx);

/* Shared replay (a live LoroDoc serves every checkout from ONE imported history and its persistent DiffCalculator,
 * crates/loro-internal/src/loro.rs:1625-1760, diff_calc.rs:62-68): entries of a staged batch that name the same blobs — the same
 * pointers and lengths, in the same order — and differ only in checkout_frontiers are ONE document rendered at several versions.
 * lm_stage uploads such a document once; every lm_run imports it once (decode, causal graph, replay from the empty version) and
 * renders each entry by moving the document's trackers to the entry's version, instead of replaying the history once per entry.
 * Results are per entry and are those of import_batch + checkout on a document of its own.  lm_import on such a batch unfolds it
 * first — every entry becomes a resident document of its own over the bytes already in HBM — and then behaves as always; so does
 * lm_richtext (the trackers have to stand at every entry's version).  Since round 6 EVERY entry with checkout_frontiers takes this
 * path, alone in its group too: the whole history is imported before the version is rendered, as LoroDoc::import + LoroDoc::checkout
 * do — damage outside the rendered version fails the entry like the reference (LM_CHECKOUT_FULL=0: the closure replay of rounds
 * 1-5).  LM_SHARE_REPLAY=0 in the environment switches the folding off.  lm_shared_documents: the
 * number of documents the batch staged last was folded into (0 = every entry is its own document, also after an lm_import). */
int lm_shared_documents(lm_ctx* ctx);

/* Diagnostics of the last lm_run (round 6).  lm_fused_documents: LWW Map documents whose blocks hold scalar writes only and were
 * resolved WITHOUT op rows — op columns folded straight into the document's LWW table (diff_calc.rs:488-616 MapDiffCalculator over
 * block_encode.rs:417-428 columns; loro_amd/csrc/lm_k_map_fused.h).  lm_redo_documents: documents (entries) the run's configuration
 * had no path for and that were replayed once more, from the staged bytes, through the span-granular batch pipeline — a delete row
 * that does not match its position under the element-granular or the resident kernels (applied by position like the reference,
 * crdt_rope.rs:256-335), a Map document the fused kernel gave up on: the verdict of a document depends neither on its neighbours
 * in the batch nor on whether the host reused blob pointers. */
int lm_fused_documents(lm_ctx* ctx);
int lm_redo_documents(lm_ctx* ctx);
/* lm_state_documents: documents of the batch staged last that were staged from their snapshot's STATE section instead of its history
 * (encoding/fast_snapshot.rs:168-258: an empty document that imports a snapshot takes its state store from that
 * section and replays nothing).  A document qualifies when it is ONE FastSnapshot blob rendered at its latest version — or ONE
 * shallow snapshot rendered at exactly its shallow root (checkout_frontiers == shallow_since_frontiers, loro_js_interop.rs:141-147),
 * or ONE snapshot + update blobs whose changes continue its history (every dependency below the snapshot's version is its
 * frontiers; loro_amd/csrc/lm_snapshot_base.h) — and every state value is of a kind this engine renders; the staged bytes are then
 * proportional to the STATE (+ the updates), the snapshot's history is neither uploaded nor decoded nor replayed, and `vv` is the
 * snapshot's own merged with what the updates add.  Updates concurrent with part of the snapshot's history need that history: such
 * a document is replayed from the snapshot's ChangeStore (same bytes out).  A later lm_import into such a batch stages the
 * snapshots once more through their ChangeStore (a history is what an import builds on).  Snapshot + updates is taken where it is the
 * cheaper replay (lm_snapshot_base.h `pays`): always when the updates are ONE chain behind the snapshot's frontiers (replayed by the
 * linear prefix: 2.2 x the rate of the history path on configs[1]-shaped documents), with concurrent branches only while the updates
 * hold at most 4,096 ops or a fifth of the history's (their deletes of base content go through the tracker's by-position path).  A
 * document staged on a state that fails in ANY way is replayed from its snapshot's history (lm_redo_documents counts it): the verdict
 * is always the history's.  LM_SNAPSHOT_STATE=0 switches the state path off, =2 takes it wherever it is possible. */
int lm_state_documents(lm_ctx* ctx);

/* Resident documents: import MORE blobs into the documents the context already holds, and / or render them
 * at other versions — what a Rust host does with
 *     doc.import(bytes)           crates/loro/src/lib.rs:710 → loro-internal/src/loro.rs:568-649,720-851 (a document with history)
 *     doc.checkout(&frontiers)    loro.rs:1625-1760;  doc.checkout_to_latest()  loro.rs:1396-1417
 * on documents it keeps alive, instead of building each one again from all its blobs.  `docs` has one entry per document of
 * the batch staged last (same count, same order): its n_blobs (possibly 0) blobs are appended to that document's history, its
 * checkout_frontiers (NULL = the latest version) is the version the next lm_run renders.  The next lm_run then
 *   - decodes the blobs and rebuilds the causal graph (the tables are per batch),
 *   - continues every sequence container's tracker from where the previous run left it (the reference keeps its trackers the
 *     same way: DiffCalculatorRetainMode::Persist, diff_calc.rs:62-68, start_tracking reuse :1371-1376): only the changes the
 *     tracker has not applied are integrated — each after the tracker moved to the change's dependencies (Tracker::checkout /
 *     forward, container/richtext/tracker.rs:350-546) — and the tracker finally moves to the version being rendered,
 *   - renders JSON + VersionVector as always.  A run that only changes the versions (no new blob anywhere) skips the decode.
 * Semantics = the sequence of calls above, NOT one import_batch of all blobs: a root Text / List whose content was visible
 * after some earlier lm_run stays part of the value when it is empty later ("text":"" — the state store never drops a
 * container state, state.rs:621-849), where one batch of the same blobs omits it.  Each lm_run is: checkout_to_latest,
 * import of the step's blobs (all of a document's blobs of one lm_import, or none: a document whose import fails — status
 * LM_DECODE_ERROR, LM_CHECKSUM_MISMATCH, LM_DATA_CORRUPTION ... — keeps exactly what it held before, loro.rs:780-838),
 * then the optional checkout; a refused checkout (LM_FRONTIERS_NOT_FOUND) does not undo the import in front of it.
 * lm_stage starts a new batch and drops everything resident.  Limits: the span-granular integrate kernel (the default);
 * a document's blobs must lie within 4 GiB of the context's blob arena; a document that holds a MovableList is replayed from
 * the empty version whenever its element layout shifts (its results are the same, its import is not incremental). */
int lm_import(lm_ctx* ctx, const lm_doc_in* docs, size_t n_docs);
/* What the reference computes before it diffs an import — the common ancestors of the version a document was at and the version
 * it reaches, and the DiffMode they imply (dag.rs:318-332,487-765 `find_common_ancestor`; oplog.rs:591-615; diff_calc.rs:72-103) —
 * computed on the device for every resident document by the last lm_run (one step = one import of all the step's blobs).
 * The version a document "was at" is the one it held after its last step that went through: a step that fails leaves it
 * there, so the step after a failed one is measured from the same version as the failed one was (the empty version if no
 * step went through yet); a step whose checkout alone was refused (LM_FRONTIERS_NOT_FOUND) went through.
 * modes[i]: 0 Checkout, 1 Import, 2 ImportGreaterUpdates, 3 Linear, -1 unknown (no resident run, failed document, more than 16
 * common-ancestor ids, a version of more than 64 heads).  lm_import_lca writes Frontiers::encode() of document `doc`'s common ancestors into buf (returns the
 * length, -1 when unknown or cap is too small).  The engine itself does not branch on the mode — its trackers hold the whole
 * history, so the replay base is wherever the tracker stands — it reports what a host that mirrors the reference needs. */
int lm_import_modes(lm_ctx* ctx, int32_t* modes);
long lm_import_lca(lm_ctx* ctx, size_t doc, uint8_t* buf, size_t cap);
/* Diagnostics: how many documents of the last lm_run could not continue from a resident tracker and were replayed from the
 * empty version (first run, capacity grown, a failed run before, MovableList layout shift). */
int lm_resident_fresh(lm_ctx* ctx);

/* Per-document metadata of the last lm_run (arrays of n_docs entries, any may be NULL) without copying the
 * rendered bytes back: what a sharded deployment all-gathers as the merged-state summary. */
int lm_result_meta(lm_ctx* ctx, int32_t* status, uint64_t* json_len, uint64_t* vv_len, uint64_t* pending_ops);
/* xxh64 (seed 0) of every document's JSON (n_docs entries; 0 for a failed document), computed on the device: the content
 * word of the merged-state summary — ranks compare merged states without moving the JSON. */
int lm_result_hashes(lm_ctx* ctx, uint64_t* json_xxh64);

/* ---- The exchange step of a sharded deployment for a host without Python: documents shard across GPUs with no
 * data-path collective; after lm_run every rank contributes the summary of its own documents — 6 int64 words per document:
 * document id, status, pending ops, JSON length, VV length, xxh64(JSON) computed on the device — and receives the table of all
 * documents of all ranks, sorted by document id, through ONE RCCL all-gather over xGMI (preceded by a one-word all-gather of the
 * shard sizes).  One process per GPU: rank 0 calls lm_comm_unique_id and hands the 128 bytes to the others out of band; every
 * rank calls lm_comm_init(ctx, rank, world, id) once (world == 1 needs neither an id nor RCCL), then lm_summary_allgather after
 * each lm_run.  RCCL is dlopen'ed at lm_comm_init; the library does not link it.  Returns rows written, -1 on error. */
int lm_comm_unique_id(uint8_t out128[128]);
int lm_comm_init(lm_ctx* ctx, int rank, int world, const uint8_t id128[128]);
long lm_summary_allgather(lm_ctx* ctx, const int64_t* doc_ids, int64_t* table, size_t cap_rows);
/* The same exchange as ONE collective on device memory.  lm_summary_layout (after lm_stage): document i of this context has the
 * global id first_id + i * stride and every rank contributes rows_padded rows (>= its document count; with documents dealt
 * `doc % world` that is ceil(total / world): computed, never exchanged).  Every lm_run then writes the rows ON THE DEVICE (rows
 * beyond the context's documents are -1): lm_summary_rows_device is that buffer — a host that drives its own collective sends it
 * as it is (bench.py: torch.distributed over RCCL) — and lm_summary_allgather_device issues the single ncclAllGather of
 * rows_padded x 6 int64 per rank and returns the gathered table (world x rows_padded rows, rank-major), which stays in device
 * memory until it is read.  lm_stage drops the layout. */
int lm_summary_layout(lm_ctx* ctx, int64_t first_id, int64_t stride, size_t rows_padded);
const int64_t* lm_summary_rows_device(lm_ctx* ctx);
long lm_summary_allgather_device(lm_ctx* ctx, const int64_t** table_dev);

/* ---- Export / encode side (host only, no device needed): the inverse of the decode stage.
 * lm_block_tables = the tables of ONE change block — the changes of one peer, counter-contiguous — exactly what the decode
 * stage extracts from a block (crates/loro-internal/src/oplog/change_store/block_encode.rs:535-706); lm_encode_block writes
 * the bytes the reference's encode_block (block_encode.rs:137-278, block_meta_encode.rs:13-88) writes for them, and
 * lm_encode_updates frames encoded blocks into a FastUpdates blob (encoding.rs:440-473, fast_snapshot.rs:346-360).  Value
 * payloads and the position arena are opaque sections: their bytes are carried as given.  Outputs are malloc'ed; release
 * them with lm_free_bytes.  Returns 0, or -1 on malformed tables. */
#include "loro_block_tables.h"   /* lm_block_tables */
int lm_encode_block(const lm_block_tables* tables, uint8_t** out, size_t* out_len);
int lm_encode_updates(const uint8_t* const* blocks, const size_t* block_lens, size_t n_blocks, uint8_t** out, size_t* out_len);
/* LoroDoc::export(ExportMode::Updates{from}) (crates/loro/src/lib.rs:1306 → encoding.rs:399-405 export_fast_updates →
 * oplog/change_store.rs:718-752 export_blocks_from) for document `doc` of the batch the context holds, after lm_run: the changes
 * its oplog holds beyond `from_vv` (VersionVector::encode() bytes, version.rs:962-968; NULL / 0 = from the empty version) as one
 * FastUpdates blob — blocks ordered by (peer, counter), blocks the version covers dropped, a block it cuts sliced at the cut
 * (the first change then depends on its peer's previous op; a run cut inside an insert / delete is sliced like the reference
 * slices it, list_op.rs:251-277,426-433).  Changes still pending are not part of the oplog and are not exported.  Host work on
 * the blobs read back from the context's arena (lm_export.h); the block boundaries are those of the imported blobs, so what was
 * staged from one writer's export comes back byte for byte from the empty version.  malloc'ed: release with lm_free_bytes. */
int lm_export(lm_ctx* ctx, size_t doc, const uint8_t* from_vv, size_t from_vv_len, uint8_t** out, size_t* out_len);
void lm_free_bytes(uint8_t* p);

/* ---- Richtext values: what TextHandler::get_richtext_value (crates/loro/src/lib.rs:2774 →
 * crates/loro-internal/src/handler.rs:1502 → container/richtext/richtext_state.rs:2546-2584) returns for every Text container of
 * the documents of the last lm_run, at the version that run rendered: a list of spans {"insert": text, "attributes": {key: value}}
 * — a scalar carries, per style key, the value of the mark (StyleOp, container/richtext.rs:31-57) with the greatest (lamport, peer)
 * among those whose StyleStart anchor stands in front of it and whose StyleEnd anchor stands behind it (style_range_map.rs;
 * state/richtext_state.rs:730-812), keys whose value is null are dropped (unmark), neighbouring spans with equal attributes are one.
 * lm_richtext renders them ON THE DEVICE (k_richtext: one wave per document over the trackers the integrate stage left) and copies
 * them back; lm_richtext_result returns document `doc`'s bytes: one JSON object {"<container id>": [span, ...], ...} over the Text
 * containers in which something (a scalar, an anchor) is visible at that version (ContainerID Display: cid:root-<name>:Text / cid:<counter>@<peer>:Text; members in the
 * bytewise order of their JSON-encoded keys), every span the canonical JSON of the LoroValue map it is ({"attributes":{...},"insert":"..."},
 * keys bytewise sorted, no "attributes" member when there are none).  *status: LM_OK, the document's import error, or
 * LM_UNSUPPORTED (more than 64 marks open at one scalar).  The bytes stay valid until the next lm_richtext / lm_stage / lm_destroy.
 * Not available on a batch folded by shared replay.  get_deep_value (lm_fetch) never shows styles: this is a call of its own. */
int lm_richtext(lm_ctx* ctx);
int lm_richtext_result(lm_ctx* ctx, size_t doc, int32_t* status, const uint8_t** json, size_t* json_len);

/* ---- Stable cursors: carets, selections, comment anchors re-anchored after a merge without a second replay on the host.  A Loro
 * `Cursor` is an element id plus a side (crates/loro-internal/src/cursor.rs); LoroDoc::get_cursor_pos resolves it
 * (crates/loro-internal/src/loro.rs:1860-1994 -> state.rs:2061-2091), TextHandler / ListHandler::get_cursor mints it
 * (handler.rs:2673-2735, 3393-3433).  Both calls are valid after lm_run and answer AT THE VERSION THAT RUN RENDERED (the latest
 * version or the entry's checkout; for resident documents the state after the last lm_import + lm_run), on the device, from the
 * trackers the run left (k_cursor: one wave per document that has queries, one pass over a container's leaves per 64 queries,
 * loro_amd/csrc/lm_k_cursor.h).  A query names its document (index into the batch staged last) and its container by the
 * ContainerID Display bytes lm_richtext_result uses as keys, unescaped: cid:root-<name>:Text, cid:<counter>@<peer>:List.
 *
 * lm_cursor_pos, per query (status, pos, pos_utf16, side):
 *   - the id is visible at that version: LM_CURSOR_OK, pos = its index among the container's visible elements — the Unicode scalar
 *     index for a Text (style anchors occupy ids but never count: the entity index -> event index conversion, handler.rs:2737-2745),
 *     the element index for a List; pos_utf16 = the same position in UTF-16 code units (one more per visible scalar >= U+10000 in
 *     front of it; == pos for a List); side is echoed (loro.rs:1875-1882);
 *   - the id is in the tracker but not visible (deleted at that version): LM_CURSOR_DELETED, pos = the number of visible elements in
 *     front of the tombstone in sequence order, side = Left (tracker.rs:608-639 get_target_id_latest_index; loro.rs:1936-1959).  The
 *     `update` cursor the reference adds is lm_cursor_at of that pos and side;
 *   - the version does not contain the id: LM_CURSOR_ID_NOT_FOUND (loro.rs:1911-1917) — a counter at or beyond that version's
 *     end for its peer, an id the checkout leaves in the future, an unknown peer, an id inside the known range that belongs to
 *     another container or to an op that creates no element (a delete, a Map write);
 *   - has_id == 0: LM_CURSOR_OK, pos = 0 for side Left, otherwise the container's length (state.rs:2073-2090).
 * An id that names a style anchor resolves to the number of visible scalars in front of the anchor (OK / DELETED like any element);
 * nothing the reference holds pins this case.
 *
 * lm_cursor_at(pos, side) — pos a Unicode scalar / element index — follows handler.rs:2704-2733:
 *   - empty container: no id, side Middle becomes Left, origin_pos 0;
 *   - pos >= len: no id, side Right, origin_pos = len;
 *   - otherwise the id of the visible element at pos, side echoed, origin_pos = pos.
 *
 * Other statuses, never a guessed position: LM_CURSOR_CONTAINER_NOT_FOUND (no such container in the document, or a key that is no
 * ContainerID), LM_CURSOR_DOC_FAILED (the document's import or checkout failed; an LM_UNSUPPORTED document that was rendered still
 * answers for its Text / List containers), LM_CURSOR_UNSUPPORTED (see Limits).  Both calls return 0, or -1 (lm_last_error) for a
 * call that cannot be answered at all: before lm_run, a document index beyond the batch, a side outside -1..1.
 *
 * Batch shapes are lm_richtext's: a batch folded by shared replay is unfolded first; documents staged from a snapshot's STATE
 * section (no element ids) are staged once more through their history and run again; documents replayed in the side engine
 * (lm_redo_documents) are answered there.  One more: the batch kernels replay a long single-writer prefix of a history as a
 * positional rope that DROPS what it deletes (the reference's unknown span has no tombstones either, tracker.rs:40-62); the first
 * cursor call on a batch that holds such a document (2,048 op rows or more) runs the batch once more with that prefix switched off
 * and the context keeps it off until the next lm_stage (a host that knows it will ask sets LM_LINEAR=0 in the environment and
 * never pays the second run; resident documents, lm_import, never go through that prefix).  In all three cases lm_fetch / lm_result_meta give the same bytes as before
 * and the calls change nothing lm_run wrote: the kernel reads tracker memory and writes only its own result rows.
 * Limits: Map, Tree and Counter containers have no element ids, a MovableList names its elements through a second id space
 * (movable_list_state.rs:941) — both LM_CURSOR_UNSUPPORTED, like every container of a document that is LM_UNSUPPORTED without a
 * rendering (a shallow snapshot, an engine limit); a Text / List container that never received an op is not in the document's
 * container table: LM_CURSOR_CONTAINER_NOT_FOUND. */
enum {
  LM_CURSOR_OK = 0,
  LM_CURSOR_DELETED = 1,
  LM_CURSOR_ID_NOT_FOUND = 2,        /* CannotFindRelativePosition::IdNotFound */
  LM_CURSOR_CONTAINER_NOT_FOUND = 3, /* CannotFindRelativePosition::ContainerDeleted / no such container */
  LM_CURSOR_DOC_FAILED = 4,
  LM_CURSOR_UNSUPPORTED = 5
};
typedef struct lm_cursor_query {
  size_t doc;               /* index into the batch staged last */
  const uint8_t* container; /* ContainerID Display bytes (not NUL terminated) */
  size_t container_len;
  int32_t has_id;           /* 0: Cursor.id == None (a cursor taken on an empty container or behind the end) */
  uint64_t peer;            /* Cursor.id */
  int32_t counter;
  int32_t side;             /* -1 Left, 0 Middle, 1 Right (cursor.rs Side) */
} lm_cursor_query;
typedef struct lm_cursor_result {
  int32_t status;           /* LM_CURSOR_* */
  uint32_t pos;             /* PosQueryResult.current.pos */
  uint32_t pos_utf16;
  int32_t side;             /* PosQueryResult.current.side */
} lm_cursor_result;
typedef struct lm_cursor_at_query {
  size_t doc;
  const uint8_t* container;
  size_t container_len;
  uint32_t pos;             /* Unicode scalar index (Text) / element index (List) */
  int32_t side;
} lm_cursor_at_query;
typedef struct lm_cursor_at_result {
  int32_t status;           /* LM_CURSOR_OK, _CONTAINER_NOT_FOUND, _DOC_FAILED, _UNSUPPORTED */
  int32_t has_id;
  uint64_t peer;            /* Cursor.id when has_id */
  int32_t counter;
  int32_t side;             /* Cursor.side */
  uint32_t origin_pos;      /* Cursor.origin_pos */
  uint32_t reserved;
} lm_cursor_at_result;
int lm_cursor_pos(lm_ctx* ctx, const lm_cursor_query* queries, size_t n, lm_cursor_result* out);
int lm_cursor_at(lm_ctx* ctx, const lm_cursor_at_query* queries, size_t n, lm_cursor_at_result* out);

/* ---- Frontiers and version vectors.  lm_fetch hands out a VersionVector and lm_delta* / lm_export take one; checkout_frontiers,
 * LoroDoc::diff / checkout / cmp_frontiers and every event of the reference speak Frontiers.  A host that offloads its imports holds
 * no DAG of its own; these two calls answer from the one the last lm_run left on the device (k_version, loro_amd/csrc/lm_k_version.h).
 *
 * lm_frontiers: the heads of document `doc` after the last lm_run as Frontiers::encode() bytes (postcard Vec<ID>, sorted), with
 * lm_import_lca's buffer convention: returns the length, -1 (lm_last_error) when there is none — before lm_run, a run in flight, a
 * document index beyond the batch, a document that failed in a batch run or has no rendering — or when `cap` is too small.
 *   which = 0: oplog_frontiers (loro.rs:1377) — the heads of everything APPLIED, whatever version was rendered;
 *   which = 1: state_frontiers (loro.rs:1382) — the heads of the version that run RENDERED (== which 0 without a checkout; a resident
 *              document whose checkout was refused stands at its latest version).
 * Computed for all documents by one launch behind the first call after a run and kept until the next run.
 *
 * lm_versions: n queries in one launch, one wave each.  Every operation is evaluated over the APPLIED history of the document, not
 * over the rendered version (the reference asks its oplog's DAG: a checked-out document still converts versions beyond its
 * checkout); pending changes are not part of that history.  By id sets: closure(id) = the id and its causal past, closure(F) = the
 * union over F, heads(S) = the ids of S that no other id of S has in its past.
 *   LM_VER_TO_VV (loro_dag.rs:1192-1207)         a = Frontiers; bytes = VersionVector::encode() of closure(a).  00 is the empty
 *       version and gives the empty vector; two ids of one peer are both taken (the greater decides).  The bytes are what lm_fetch
 *       returns as `vv` when that version is checked out: pass them as from_vv to lm_delta* / lm_export as they are.
 *   LM_VER_TO_FRONTIERS (loro_dag.rs:1269-1298)  a = VersionVector; bytes = Frontiers::encode() of heads({(p, a[p] - 1) : a[p] > 0}).
 *       Entries of 0 (or below) are skipped.  The vector need not be causally closed: this is the shrink of its last ids.
 *   LM_VER_MINIMIZE (lib.rs:855)                 a = Frontiers; bytes = Frontiers::encode() of heads(a).
 *   LM_VER_CMP (loro_dag.rs:1347-1355)           a, b = Frontiers; order = -1 / 0 / 1 for closure(a) a proper subset of / equal to /
 *       a proper superset of closure(b), 2 when neither contains the other.
 *   LM_VER_CMP_DOC (loro_dag.rs:1333-1341)       a = Frontiers; order = 0 when a equals the document's oplog frontiers as a set of
 *       ids; else 1 when the applied vector includes every id of a (a vector test, no DAG lookup); else -1 ("less or parallel": an
 *       unknown id lands here and is no error).
 * Statuses: LM_FRONTIERS_NOT_FOUND (all but CMP_DOC) — an id outside the applied history: an unknown peer, a counter at or beyond the
 * peer's applied end, a negative counter, an id inside a pending change; for TO_FRONTIERS an entry above 0 of an unknown peer or beyond
 * the applied end.  LM_DECODE_ERROR — bytes that are not a Frontiers / a VersionVector (truncated, bytes left over, zero length: the
 * empty version is the byte 00).  The document's own import error for a failed document, LM_UNSUPPORTED for one without a rendering
 * (an engine limit, a shallow snapshot); a document that only carries Tree / Counter containers beside the rest answers normally.
 * Returns 0, or -1 (lm_last_error) before lm_run, during a run in flight, for a document index beyond the batch or an op outside the
 * enum.  Batch shapes: a document staged from a snapshot's STATE section is staged once more through its history and run again; a
 * batch folded by shared replay is UNFOLDED by the first call (which = 1 needs every entry's own rendered version; every entry then
 * holds the one applied history, so which = 0 and lm_versions answer alike for the entries of one document); documents replayed in
 * the side engine are answered there; resident documents answer for the state after the last lm_import + lm_run.
 * After a FAILED step a resident document stands where it stood before, and so do its heads: lm_frontiers gives, both ways, what
 * it gave after the document's last step that went through (the byte 00 when none did yet), unchanged until a step goes through
 * and moves them on.  (Kept from the tables of the run before: a run that brings new blobs computes the heads in front of its
 * decode stage unless a call already has; a run that only moves the rendered versions pays nothing, and a document such a run
 * fails for has no heads: -1.)  lm_versions has no tables for that document — the failed run built none — and answers the step's
 * error for it until a step goes through.
 * The calls change nothing a run wrote: lm_fetch, lm_result_meta and lm_import_modes give the same bytes afterwards.
 * LoroDoc::diff(a, b): check out b, LM_VER_TO_VV(a), lm_delta* (INTEGRATION.md). */
long lm_frontiers(lm_ctx* ctx, size_t doc, int which, uint8_t* buf, size_t cap);
enum { LM_VER_TO_VV = 0, LM_VER_TO_FRONTIERS = 1, LM_VER_MINIMIZE = 2, LM_VER_CMP = 3, LM_VER_CMP_DOC = 4 };
typedef struct lm_version_query {
  size_t doc;               /* index into the batch staged last */
  int32_t op;               /* LM_VER_* */
  const uint8_t* a;         /* Frontiers::encode() bytes; LM_VER_TO_FRONTIERS: VersionVector::encode() bytes */
  size_t a_len;
  const uint8_t* b;         /* LM_VER_CMP: the second Frontiers; unused otherwise */
  size_t b_len;
} lm_version_query;
typedef struct lm_version_result {
  int32_t status;           /* LM_OK | LM_FRONTIERS_NOT_FOUND | LM_DECODE_ERROR | the document's import error | LM_UNSUPPORTED */
  int32_t order;            /* LM_VER_CMP: -1 / 0 / 1 / 2; LM_VER_CMP_DOC: -1 / 0 / 1; 0 otherwise */
  const uint8_t* bytes;     /* TO_VV / TO_FRONTIERS / MINIMIZE; valid until the next lm_versions / lm_stage / lm_destroy */
  size_t len;
} lm_version_result;
int lm_versions(lm_ctx* ctx, const lm_version_query* queries, size_t n, lm_version_result* out);

/* ---- Text and List deltas between two versions: what changed since the version this subscriber has?  LoroDoc::diff(a, b) and the
 * TextDelta / ListDiffItem events of subscribe, answered on the device from the trackers and the decoded op rows the run left
 * (k_delta_mark, k_delta: loro_amd/csrc/lm_k_delta.h) instead of a fetch of the whole JSON and a string diff on the host — which
 * cannot even tell which of two equal characters was deleted.  Valid after lm_run; a query answers from A = from_vv to V = THE
 * VERSION THAT RUN RENDERED (the latest version, the entry's checkout, a resident document's state after the last lm_import +
 * lm_run).  Several queries may name the same document: subscribers stand at different versions.
 *
 * Definition, by id sets (exact, and independent of how the tracker got where it stands: A may be any version V contains).  For
 * one Text or List container take its elements in the tracker's sequence order, which does not depend on the version:
 *   - an element (p, c) is in A iff c < A[p] and no delete atom whose own id lies in A targets it;
 *   - it is in V iff it is visible at the rendered version;
 *   - style anchors are never elements of a delta;
 *   - K = in both, I = in V only, D = in A only, everything else is skipped.
 * Canonical delta of a container: a maximal run of K gives {"retain":n}; the I and D elements between two K runs (or a container
 * edge), however interleaved, give at most one {"insert":...} holding all I of the gap in sequence order, followed by at most one
 * {"delete":n} counting its D; a trailing retain is dropped; an empty delta leaves the container out.
 * Payloads: a Text insert is a JSON string escaped exactly as lm_fetch's JSON escapes Text values; a List insert is a JSON array of
 * the elements' values in the same canonical form; an element that is a child container is the JSON string of the parrot prefix
 * U+1F99C ':' + its ContainerID Display (LoroValue::Container, loro-common/src/value.rs:717) — the child's content is never
 * inlined, its delta stands under its own key.  With units == 1 a Text retain / delete counts one more per scalar >= U+10000.
 * Result bytes of a query: one JSON object {"<ContainerID Display>":[op,...],...} over every Text / List container of the document
 * whose delta is not empty, members in the bytewise order of their JSON-encoded keys (lm_richtext_result's rule); {} when nothing
 * changed.  Attributes are out of scope: lm_richtext gives the styles at V, lm_delta_richtext below the delta with attributes.
 *
 * Statuses: LM_FRONTIERS_NOT_FOUND — some A[p] > V[p], or A names a peer the document does not know with a counter > 0;
 * LM_UNSUPPORTED — the document has no rendering (an engine limit), or the kernel's self-check failed ("visible by status" must
 * equal "c < V[p] and not deleted by an id in V" for every element; a mismatch is a delete applied by position, a damaged document
 * or anything not thought of): the right value or a refusal, never a guess.  Returns 0, or -1 (lm_last_error) for a call that
 * cannot be answered at all: before lm_run, during a run in flight, a document index beyond the batch, units outside 0..1.
 * Batch shapes are the cursor calls' (folded batches are unfolded, state-staged snapshots staged once more through their history,
 * side-engine documents answered there, a batch with a document that went through the linear prefix run once more keeping its
 * tombstones).  Only the bytes a query's answer holds cross to the host (lm_delta_bytes).  The call changes nothing a run wrote: lm_fetch / lm_result_meta give the same bytes afterwards. */
typedef struct lm_delta_query {
  size_t doc;               /* index into the batch staged last */
  const uint8_t* from_vv;   /* VersionVector::encode() bytes — what lm_fetch returned as `vv` at the earlier step, the same
                               format lm_export takes; NULL / 0 = the empty version */
  size_t from_vv_len;
} lm_delta_query;
typedef struct lm_delta_result {
  int32_t status;           /* LM_OK | the document's import error | LM_DECODE_ERROR (from_vv is not a VersionVector) |
                               LM_FRONTIERS_NOT_FOUND (from_vv is not contained in the rendered version) | LM_UNSUPPORTED */
  uint32_t other_changed;   /* 1: a container of a kind this call does not cover (Map, MovableList, Tree, Counter) received an op
                               whose id lies in V \ A — the host falls back to the rendering for those */
  const uint8_t* json;      /* valid until the next lm_delta / lm_stage / lm_destroy */
  size_t json_len;
} lm_delta_result;
/* units: 0 = Text counts in Unicode scalars, 1 = in UTF-16 code units (List counts are elements either way) */
int lm_delta(lm_ctx* ctx, const lm_delta_query* queries, size_t n, int units, lm_delta_result* out);
/* Bytes the last lm_delta copied from the device to the host: 16 bytes of result row per query and launch, plus the queries' JSON
 * packed on the device (each rounded up to 16 bytes) — proportional to the change, never to the documents. */
uint64_t lm_delta_bytes(lm_ctx* ctx);

/* ---- Map deltas from a version to the rendered one: what LoroDoc::diff(a, b) and the MapDelta events of subscribe tell a subscriber
 * about the Map containers (diff_calc.rs:545-610 over get_container_latest_op_at_vv), answered on the device from the LWW tables and
 * op rows of the last lm_run (k_mdelta_mark, k_mdelta: loro_amd/csrc/lm_k_delta_map.h).  Same query and result structs as lm_delta,
 * no `units`; valid in the same states, the same -1 for a call that cannot be answered, the same batch shapes.  A = from_vv, V = the
 * version that run rendered (the latest version, the entry's checkout, a resident document's state).
 *
 * Definition.  For one Map container and one key a WRITE is a Map set or Map delete op of an applied change (beyond a sliced
 * change's known prefix).  The winner at a version X is the write with the greatest (lamport, peer id) among the writes whose id
 * lies in X (counter < X[peer]); "no write in X" is a state of its own, distinct from a winning delete.  With wA / wV the winners
 * at A / V:
 *   - wV absent: nothing (cannot be when A is contained in V and something is reported);
 *   - wA and wV are the same op: nothing;
 *   - wA absent: reported — wV a set goes to "updated", wV a delete to "deleted" (the reference pushes every key that is only in
 *     the target map, a delete included);
 *   - both deletes: nothing; exactly one a delete: reported;
 *   - both sets: reported iff the values differ under LoroValue equality (loro-common/src/value.rs:29-44): different kinds differ
 *     (I64 3 against F64 3.0); Null, Bool, I64 by value; F64 as a == b || (a.is_nan() && b.is_nan()), so 0.0 equals -0.0 although
 *     their JSON differs; String and Binary by bytes; a child container is the ContainerID of its creating op, two ops are never
 *     equal.  Two nested List values, or two nested Map values, from different ops are NOT decided on the device (nested Map values
 *     name keys through their block's key table; JSON equality parts from LoroValue equality on +-0.0 and Binary against List):
 *     the key is left out and bit 1 of other_changed is set — the right value or a refusal, never a guess.
 * other_changed of this call: bit 0 — an op with an id in V \ A went to a MovableList, Tree or Counter container; bit 1 — an
 * undecided nested pair.  Text and List ops set nothing (lm_delta covers them).
 * Result bytes of a query: one JSON object over every Map container of the document whose delta is not empty — decided by id sets: a
 * child Map hidden by a later write to its parent's key is still listed under its own ContainerID —
 *   {"<ContainerID Display>":{"updated":{"<key>":<value>,...},"deleted":["<key>",...]},...}
 * both members always present; keys inside "updated" and "deleted" in the bytewise order of their raw bytes (lm_fetch's order),
 * escaped as lm_fetch escapes them; values in lm_fetch's canonical form; a child container is the parrot string (U+1F99C ':'
 * ContainerID Display) as in lm_delta, its content stands under its own key; containers in the bytewise order of their JSON-encoded
 * keys; {} when nothing changed.
 * Statuses: lm_delta's.  LM_UNSUPPORTED also when the kernel's self-check failed: the winner at V found from the op rows must equal
 * the winner the run's LWW stage left in the document's table, for every key.  A document that was decoded without op rows (an LWW
 * Map document, lm_fused_documents) is run once more through the row tables first; lm_fetch gives the same bytes afterwards.
 * lm_delta_bytes reports the bytes of whichever of lm_delta / lm_delta_map ran last; `json` is valid until the next lm_delta /
 * lm_delta_map / lm_stage / lm_destroy.  The call changes nothing a run wrote. */
int lm_delta_map(lm_ctx* ctx, const lm_delta_query* queries, size_t n, lm_delta_result* out);

/* ---- MovableList deltas from a version to the rendered one: what LoroDoc::diff(a, b) and the ListDiffItem events of subscribe tell a
 * subscriber about the MovableList containers (movable_list_state.rs:1136-1183, event.rs:244-250), answered on the device from the
 * trackers, the table of move / set maxima and the op rows of the last lm_run (k_mldelta_mark, k_mldelta:
 * loro_amd/csrc/lm_k_delta_movable.h).  Same query and result structs as lm_delta, no `units`; valid in the same states, the same -1
 * for a call that cannot be answered (before lm_run among them), the same batch shapes.  A = from_vv, V = the version that run
 * rendered (the latest version, the entry's checkout, a resident document's state); A is contained in V as id sets.
 *
 * Definition, for one MovableList container.
 *   - Items.  Every atom of an insert op and every move op is an ITEM whose id is that op's id; el(i) is the element it positions (an
 *     element is what an insert atom created).  The items stand in the tracker's sequence order, which does not depend on the version.
 *   - Position.  pos_X(e) = the greatest, by (lamport, peer id), of e's insert and its moves whose ids lie in X.
 *   - Value.  val_X(e) = the greatest, by the same order, of e's insert and its sets in X.
 *   - Item i SHOWS at X iff id(i) is in X, i is pos_X(el(i)), and no delete atom whose own id lies in X targets i.  (A move also
 *     removes the item it took the element from; the winner of X is never such an item, so nothing more is needed.)
 *   - Value unchanged for e between A and V: val_A(e) and val_V(e) are the same op, or different ops whose values are equal under
 *     LoroValue equality as lm_delta_map compares them.  A pair that comparison does not decide (two nested List values, two nested
 *     Map values) counts as CHANGED and sets bit 1 of other_changed: the delta stays correct, it is only less minimal.
 *   - Classes per item.  K: shows at A and at V, value unchanged.  R: shows at both, value changed — one delete and one insert in
 *     place.  I: shows at V only.  D: shows at A only.
 *   - from_move.  An I carries "from_move" iff its element shows at A (necessarily at another item, which is then a D) and its value
 *     is unchanged: "moved from a deletion in the same delta and the value is not changed".
 * Canonical form (lm_delta's): a maximal K run gives {"retain":n}; within a gap all inserts come first, in sequence order, consecutive
 * inserts with the same flag in one op — {"insert":[v,...]} or {"insert":[v,...],"from_move":true} — then one {"delete":n}; a trailing
 * retain is dropped; a container with an empty delta is left out; containers in the bytewise order of their JSON-encoded keys; values
 * in lm_fetch's canonical form; a child container is the parrot string (U+1F99C ':' ContainerID Display) of the ContainerID of the op
 * that wrote it (the winning set, else the insert).  Result bytes of a query:
 *   {"cid:root-ml:MovableList":[{"delete":1},{"retain":2},{"insert":["a"],"from_move":true}],...}        {} when nothing changed.
 * other_changed of this call: bit 0 — an op with an id in V \ A went to a Tree or Counter container; bit 1 — an undecided nested pair
 * was treated as changed.  Text, List and Map ops set nothing (lm_delta and lm_delta_map cover them).
 * A document that holds Tree or Counter ops is one lm_fetch reports as LM_UNSUPPORTED together with its JSON; that status is the
 * rendering's, not this call's: the query comes back LM_OK with the MovableList deltas, and bit 0 tells the host that the part of the
 * document the device does not render changed as well.
 * Statuses: lm_delta's (LM_DECODE_ERROR: from_vv is no version vector; LM_FRONTIERS_NOT_FOUND: A is not contained in V).
 * LM_UNSUPPORTED also when the kernel's self-check failed — for every item "visible by the tracker's status word" must equal "id in V
 * and not removed by a delete or move in V", and for every element the move and set winners at V found from the op rows must be the
 * ops the run left in the document's table — or when a slot lies beyond the call's bitmaps or tables.  A = V, an LWW Map document
 * decoded without op rows, and a document that holds neither a MovableList nor an applied Tree / Counter op are answered {} on the host.
 * lm_delta_bytes reports the bytes of whichever of lm_delta / lm_delta_map / lm_delta_movable ran last; `json` is valid until the next
 * of these calls / lm_stage / lm_destroy.  The call changes nothing a run wrote: lm_fetch gives the same bytes afterwards. */
int lm_delta_movable(lm_ctx* ctx, const lm_delta_query* queries, size_t n, lm_delta_result* out);

/* ---- Text deltas WITH STYLE ATTRIBUTES from a version to the rendered one: what the TextDelta events of subscribe tell a rich-text
 * subscriber — lm_delta's answer for the Text containers, its retains and inserts carrying attributes.  The call is to lm_delta what
 * lm_richtext is to lm_fetch; answered on the device from the trackers, the anchors' StyleOps and the op rows of the last lm_run
 * (k_rtdelta_mark, k_rtdelta: loro_amd/csrc/lm_k_delta_richtext.h).  lm_delta's query and result structs, `units`, valid states, -1
 * cases, batch shapes and the lifetime of `json`.  Text containers only.  A = from_vv, V = the version that run rendered.
 *
 * Definition, by id sets, for one Text container; its elements, anchors included, stand in the tracker's sequence order.
 *   - Scalars are classed K / I / D / skipped exactly as lm_delta classes them.  Anchors are never elements of a delta.
 *   - A MARK is a StyleStart anchor (p, c) together with its StyleEnd (p, c + 1); it carries the StyleOp (key, value, lamport, peer)
 *     of the Start.  It is live at A iff both anchors are in A by lm_delta's own test (counter below A[p], no delete atom in A
 *     targets the slot); live at V iff both anchors are visible; in both cases the End stands behind the Start.  A version that
 *     contains the Start and not the End has no such mark.
 *   - attrs_X(s), X one of A / V, for a scalar s: per key, the value of the mark live at X with the greatest (lamport, peer id) among
 *     those whose Start stands in front of s and whose End stands behind it; a key whose winner has a null value is absent.
 *   - An I scalar carries attrs_V.  A D scalar carries nothing.  A K scalar carries its CHANGE SET: key: attrs_V[key] for every key
 *     that attrs_A lacks or whose two values are unequal under LoroValue equality (loro-common/src/value.rs:29-44, as lm_delta_map
 *     compares them), key: null for every key in attrs_A and not in attrs_V.  When the same op wins a key at A and at V the key is
 *     unchanged and no values are compared.
 * Canonical form: lm_delta's, with runs also cut by attributes.  A maximal run of K scalars — anchors and skipped elements between
 * them do not count — whose neighbouring change sets are equal (equal key sets, equal values per key; a joined run keeps the set it
 * was opened with) gives {"retain":n} or {"attributes":{...},"retain":n}.  A gap gives first its I scalars in sequence order, one
 * {"insert":"..."} or {"attributes":{...},"insert":"..."} per maximal run of equal attrs_V, then at most one {"delete":n}.  A trailing
 * retain WITHOUT attributes is dropped, one with attributes stays.  A container with an empty delta is left out; {} when nothing
 * changed; members in the bytewise order of their JSON-encoded keys; attribute keys bytewise sorted and escaped, values in the
 * canonical form, as lm_richtext writes them; units == 1 counts as in lm_delta.
 * Nested values: two nested List / Map values from DIFFERENT ops are not compared on the device (the rule of lm_delta_map /
 * lm_delta_movable): in a change set the key counts as changed and carries V's value, in a run join the runs stay apart, and bit 1 of
 * other_changed is set — still a correct delta, only not a minimal one.
 * other_changed of this call: bit 0 — a List, Map, MovableList, Tree or Counter container received an op whose id lies in V \ A;
 * bit 1 — an undecided nested pair.
 * Statuses: lm_delta's; LM_UNSUPPORTED also when more than 64 marks are live at one place at A or at V, when a Text has more than 64
 * distinct style keys, or when lm_delta's self-check fails.
 * Relation to the reference: its own events (richtext_state.rs:379-560) are not minimal — on a deleted anchor it annotates the whole
 * affected range again with every style it carries, and its inserts go through to_option_map, which keeps null-valued keys.  This
 * call gives the minimal delta, with nulls dropped from inserts; applying either to the rich-text value at A gives the rich-text
 * value at V.  Byte equality with a Rust event is not claimed.
 * lm_delta_bytes reports whichever delta call ran last.  The call changes nothing a run wrote. */
int lm_delta_richtext(lm_ctx* ctx, const lm_delta_query* queries, size_t n, int units, lm_delta_result* out);

/* Wave-primitive self test on the device (DPP scan, ballot ranks); returns the number of mismatches. */
int lm_selftest(lm_ctx* ctx);

/* Introspection for bench.py: byte counts of the last run and per-kernel HIP-event timings. */
typedef struct lm_run_stats {
  uint64_t n_docs, n_blobs;
  uint64_t in_bytes;   /* Σ blob lengths */
  uint64_t out_bytes;  /* Σ json_len + Σ vv_len */
  uint64_t device_bytes_allocated;
  uint32_t n_kernels;
} lm_run_stats;
int lm_get_stats(lm_ctx* ctx, lm_run_stats* out);
int lm_set_profiling(lm_ctx* ctx, int mode);                  /* hipEvents around every stage of lm_run (recorded without
                                                                * host syncs): 0 off | 1 and the context's streams run one after
                                                                * the other (a stage's own duration) | 2 streams overlapped as
                                                                * usual (durations as they occur in production) */
int lm_kernel_time(lm_ctx* ctx, uint32_t i, const char** name, double* ms); /* i < n_kernels, after lm_run */
/* A context splits a staged batch into contiguous document ranges, one engine on its own HIP stream each
 * (env LM_STREAMS, default 2; batches under 128 documents per stream stay whole) and lm_run drives them from
 * separate host threads so the stages of different ranges overlap on the device.  Returns the split of the
 * batch staged last.  lm_kernel_time lists the stages of every stream (same names, one entry per stream). */
int lm_n_streams(lm_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
