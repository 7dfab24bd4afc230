// Decode stage: envelope + checksum, change-block framing, columnar op tables.
// Follows the reference decoder (paths relative to /root/reference/crates/loro-internal/src):
//   parse_header_and_body / checksum   encoding.rs:302-373
//   decode_updates                      encoding/fast_snapshot.rs:372-400
//   EncodedBlock                        oplog/change_store/block_encode.rs:94-119
//   decode_changes_header               oplog/change_store/block_meta_encode.rs:90-242
//   EncodedOp columns + row walk        oplog/change_store/block_encode.rs:417-445,651-704
//   decode_op / delete start ids        encoding/outdated_encode_reordered.rs:215-476,480-489
//   value payloads                      encoding/value.rs:342-459,608-859 (docs/encoding.md §10)
#pragma once
#include "lm_dev_util.h"

namespace lm {

struct Dev {  // device pointers of one batch (passed by value to every kernel)
  // inputs
  const uint8_t* data;
  const uint64_t* blob_off;   // [n_blobs] 16-byte aligned start of each blob
  const uint32_t* blob_len;   // [n_blobs] exact byte length
  const uint32_t* doc_blob;   // [n_docs+1] first blob of each doc
  uint32_t n_blobs, n_docs;
  uint32_t span;              // 1: leaves hold runs (lm_k_integrate_span.h, SP_REC dwords per leaf), 0: one element per slot
  const uint32_t* res_old_blobs;   // resident documents: per document the number of blobs earlier runs already held (nullptr otherwise)
  uint32_t loc_cleared;       // 1: kept[] was set to 0 by a fill in front of the integrate stage (the waves skip their own clear)
  uint32_t* posdel;           // per document 3 * PD_CAP words: the delete rows the span-granular batch kernels applied by position (lm_k_integrate_span.h ts_del_positional); nullptr = a mismatch is LM_DATA_CORRUPTION
  const uint64_t* posdel_off; // per document (n_docs + 1): its slice of `posdel` in pieces; nullptr = PD_CAP pieces each
  uint32_t* pd_row_idx;       // per op row of the batch: the first piece of a row applied by position in its document's list (documents whose slice exceeds PD_CAP: staged on a snapshot's state); nullptr = no such document
  const uint8_t* vvo;         // per document: the version vector to write out instead of the decoded peers' (a document staged from a snapshot's STATE section, lm_snapshot.h); vvo_off[n_docs + 1], empty range = none; nullptr = no such document
  const uint64_t* vvo_off;
  const uint8_t* doc_fused;   // per document: 1 = an LWW Map document decoded without op rows (lm_k_map_fused.h; nullptr: none in this run)
  uint32_t n_op_rows;         // op rows of the batch's row tables (the fused documents' record tables start behind them)
  uint32_t* blk_kind;         // per block (k_block_kind): bit 31 = Map ops with scalar values only, low bits = its op rows
  uint32_t posdel_redo;       // 1: a replay without a positional delete path (element-granular kernel, resident kernels of a folded batch) flags a document that needs one DF_REDO — the context replays it through the span-granular batch kernels (lm_capi_impl.h)
  uint32_t no_linear;         // 1 (LM_LINEAR=0): no linear prefix — every node of a plain document goes through the tracker (lm_k_integrate_linear.h; A/B runs)
  uint32_t res_vis;           // 1: resident documents — the trackers stand at the rendered version, an item shows iff it is active
  const uint8_t* front;       // optional checkout frontiers (postcard Vec<ID>), front_off[n_docs+1]; empty range = latest
  const uint64_t* front_off;
  const uint8_t* froot;       // per document: root containers its first snapshot's state section holds ([kind, uleb len, name]*)
  const uint64_t* froot_off;
  // per blob
  int32_t* blob_status;
  uint32_t* blob_hash;        // xxh32 of the large blobs (k_hash_big_blobs)
  uint32_t* blob_nblk;
  uint32_t* blob_blk0;
  uint32_t* blob_doc;
  // per block
  uint32_t n_blocks;
  BlockDesc* blk;
  uint32_t* bcnt;   // [n_blocks+1][BCN] counts, then exclusive offsets in boff
  uint32_t* boff;
  // rows
  ChangeRow* chg;
  uint32_t* dep_peer;
  uint32_t* dep_ctr;
  uint32_t* dep_ci;      // per dep row: the sorted applied change (doc-relative index into chg_sorted) that holds the dependency, NONE if none — resolved once by k_dag_a, read by k_dag_b
  OpRow* op;
  uint64_t* op_val;
  uint32_t* op_blk;
  uint64_t* key_off;
  uint32_t* key_len;
  uint32_t* cid_raw;   // 4 words per raw cid: kind|root<<8, peer local idx, key idx / counter, block
  uint32_t* cid_map;   // raw cid row → doc container idx
  uint64_t* peer_raw;  // per block peer tables
  uint32_t* peer_map;  // raw peer row → doc peer idx
  // per doc
  DocMeta* doc;
  const uint32_t* doc_order;   // integrate stage: workgroup → document, longest (most op rows) first
  uint64_t* peer_uniq;   // [praw0 + i], i < n_peers, ascending
  uint32_t* peer_end;    // applied (exclusive) counter end == final VV; lowered to the checkout version by k_dag_b
  uint32_t* peer_ext;    // contiguous covered end
  uint32_t* peer_base;   // the peer's end in the document's BASE version (k_dag_a: 0 unless the document is staged on a snapshot's state, Dev::vvo) — every version of the document holds at least this
  uint32_t* peer_end_all;// checked-out documents: the applied end at the LATEST version (peer_end before k_dag_b lowered it)
  uint32_t* elem_base;   // first element slot of the peer inside the doc's element range
  uint32_t* elem_cap;    // resident documents: element slots the peer's region holds (k_res_layout)
  uint32_t* peer_chg0;   // range of the peer's changes in chg_sorted
  uint32_t* peer_chg1;
  ContRow* cont;         // [cid0 + i], i < n_cont
  // dag
  uint32_t* chg_sorted;  // [chg0 + i] → global change row
  uint32_t* chg_lamport; // per global change row
  uint32_t* chg_skip;    // atoms to skip at the start of a change (already known prefix)
  uint32_t* chg_flag;    // 1 = applied
  uint32_t* chg_mask;    // per change 2 words: bit (container idx & 63) set for every container its ops touch
  uint32_t* node_first;  // [chg0 + n] indices into chg_sorted (doc-relative)
  uint32_t* node_last;
  uint32_t* node_order;  // replay order (doc-relative node ids)
  uint32_t* vvh;         // [vvh0 + node*P + p]
  // elements
  uint32_t* cp;          // text: unicode scalar (CP_ANCHOR | op row = style anchor) | list: value offset rel. to the doc's first byte
  uint32_t* loc;         // element → leaf
  uint32_t* kept;        // span-granular kernels: bit (slot & 31) of word (slot >> 5) = loc[slot] holds a kept entry (lm_k_integrate_span.h sp_keep)
  uint32_t* dcnt;        // resident documents: element → delete ops of the version a tracker is being moved to (ts_sweep_version); nullptr otherwise
  uint8_t* tb;           // span-granular leaves: one byte per Text element — the scalar when it is ASCII, TB_WIDE: cp[] holds it, TB_ANCHOR: a style anchor
  // tracker pools
  uint32_t* it;          // leaf records, 256 dwords each: id[64] | origin_left[64] | origin_right[64] | status[64]
  uint8_t* lf_chunk;     // [leaf0 + leaf] chunk (owning lane) of the leaf's directory entry
  uint32_t* dir_out;     // [leaf0 + i] flushed leaf directories (entry = leaf | n<<18 | act<<25)
  uint32_t* cont_root0;  // per doc container: first directory entry (doc-relative) / number of entries
  uint32_t* cont_nroot;
  // map LWW
  unsigned long long* ht_key;   // per doc open-addressing table
  unsigned long long* ht_best;
  unsigned long long* ht_pfx;   // per slot: first eight key bytes (big endian), filled by the emit stage for its key sort
  uint64_t* ht0;                // per doc first slot; ht_cap per doc
  uint32_t* ht_cap;
  uint32_t* ht_list;            // per doc [ht0, ht0+cap): lower half = slots claimed (one per distinct key), upper half = sort scratch
  uint32_t* ht_cnt;             // per doc number of claimed slots
  unsigned long long* prof;     // [doc*16 + slot] cycle accounting (LM_PROF builds)
  uint32_t* fuse;               // [2 x op row] k_fuse_rows: a run head's leftmost delete target counter | signed total length (nullptr: no run was chained)
  uint32_t* dec_stat;           // [0] blocks whose head (everything before the value payloads) exceeds dec_slot bytes, [1] the largest such head, [2] the largest span of such a block's op / delete-start columns
  uint32_t dec_slot;            // the decoder's default LDS slot (k_block_count compares against it)
  uint32_t vs_row_cost;         // ts_sweep_pays_batch: what a row-by-row tracker move costs per op row, in the units of the pass's cost estimate
  uint32_t cut_min_rows;        // k_dag_a: documents of at least this many op rows get the node cut + descending-peer replay order (DF_CUT)
  // outputs
  uint8_t* out;          // JSON bytes
  uint64_t* out_off;     // per doc offset (n_docs+1)
  uint8_t* vv_out;
  uint64_t* vv_off;
};
static constexpr int BCN = 8;  // counters per block: chg, dep, op, key, cid, peer, mapop, atoms
enum { BC_CHG = 0, BC_DEP, BC_OP, BC_KEY, BC_CID, BC_PEER, BC_MAPOP, BC_ATOMS };
static constexpr uint32_t VIS_CAP = 1024;
static constexpr uint32_t TB_WIDE = 0xFF, TB_ANCHOR = 0xFE;   // Dev::tb markers (neither is a byte of an ASCII scalar)
static constexpr uint32_t CP_ANCHOR = 0x80000000u, CP_ALIVE = 0x40000000u;   // Dev::cp of a style anchor: CP_ANCHOR | op row inside the document (no unicode scalar has bit 31); CP_ALIVE: k_richtext's mark while it runs

// -------------------------------------------------------------------------------------------------
static constexpr uint64_t BIG_BLOB = 32768;   // blobs from this size on are hashed by a whole wave
// K0: the envelope checksum of the large blobs (listed by the host, which knows the blob lengths, longest first) — FOUR blobs per
// wave, one per 16-lane row.  xxh32's four accumulators are a serial chain by construction (add, rotate, multiply per 16-byte
// stripe: ≈1.5 ms for a 2.4 MB blob whatever runs beside it), so what a kernel can do about it is (1) never wait for memory inside
// the chain and (2) spend few instructions per byte:
//  * a row's 16 lanes load one 64-byte chunk per instruction (lane 4j+a: word a of stripe j) and lanes 0..3 — the accumulators —
//    take the other lanes' words through the DPP crossbar (row_shl 4 / 8 / 12, no LDS);
//  * three register banks of 1 KB per blob rotate: while one bank is consumed, the loads of the next two are in flight (2 KB per
//    blob ahead of the chain — the chain needs 0.64 µs per KB, a load ≈1.5 µs).
// Rounds 2-4a: one wave per blob, the KB loaded and waited for in front of its 64 chain steps, every step fed by an LDS permute
// (≈5 ms per 2.4 MB blob, 6.9 ms for a configs[2] batch of 2,048 documents); a first 16-blobs-per-wave version with a dword per
// lane and stripe kept only 128 bytes per blob in flight and measured 21 ms.
static constexpr uint32_t HASH_G = 4;
LM_DEV uint32_t xx_round(uint32_t v, uint32_t m) { return rotl32(v + m, 13) * 0x9E3779B1u; }
LM_KERNEL LM_WAVES_PER_SIMD(2) LM_ONE_WAVE_GROUPS void k_hash_big_blobs(Dev d, const uint32_t* big, uint32_t n_big) {
  const uint32_t P1 = 0x9E3779B1u, P2 = 0x85EBCA77u, P3 = 0xC2B2AE3Du, P4 = 0x27D4EB2Fu, P5 = 0x165667B1u;
  const uint32_t seed = 0x4f524f4cu;
  uint32_t lane = (uint32_t)lmw::lane(), row = lane >> 4, rl = lane & 15, a = lane & 3;
  uint32_t i = (uint32_t)lmw::bid() * HASH_G + row;
  bool have = i < n_big;
  uint32_t b = big[have ? i : 0u];                       // (a row without a blob reads the first listed blob's first KB and keeps nothing)
  uint64_t blen = have ? d.blob_len[b] : 0ull;
  uint64_t len = blen >= 1024 + 20 ? blen - 20 : 0ull;   // (listed blobs are >= BIG_BLOB bytes; anything shorter hashes to 0)
  const uint8_t* p = d.data + d.blob_off[b] + 20;        // blob starts are 16-byte aligned: p is 4-byte aligned
  const uint32_t* w = (const uint32_t*)p + rl;           // this lane's word of every 64-byte chunk
  uint32_t v = a == 0 ? seed + P1 + P2 : a == 1 ? seed + P2 : a == 2 ? seed : seed - P1;
  const uint32_t n_str = (uint32_t)(len >> 4), n_kb = n_str >> 6;   // stripes, whole KBs (a blob is shorter than 4 GiB)
  const uint32_t T = lmw::reduce_max(n_kb);              // trips of the wave: its longest blob's
  uint32_t xa[16], xb[16], xc[16];
  // (every load is unconditional — a lane past its blob's last KB reads that KB again and the chain drops the result: a load under
  // a lane predicate becomes a branch with a wait for memory behind it, sixteen of them per KB)
  const uint32_t kb_last = n_kb ? n_kb - 1 : 0u;
#define LM_HASH_LOAD(x, t) do { const uint32_t* q_ = w + (size_t)256 * ((t) < kb_last ? (t) : kb_last); _Pragma("unroll") for (int k_ = 0; k_ < 16; k_++) x[k_] = q_[16 * k_]; } while (0)
#define LM_HASH_CHAIN(x, t) do { uint32_t nv_ = v; _Pragma("unroll") for (int k_ = 0; k_ < 16; k_++) { const uint32_t m_ = x[k_] * P2; \
      nv_ = xx_round(nv_, m_); nv_ = xx_round(nv_, lmw::row_down<4>(m_)); nv_ = xx_round(nv_, lmw::row_down<8>(m_)); nv_ = xx_round(nv_, lmw::row_down<12>(m_)); LM_SCHED_FENCE(); } \
    if ((t) < n_kb) v = nv_; } while (0)
  LM_HASH_LOAD(xa, 0u); LM_HASH_LOAD(xb, 1u);
#pragma unroll 1
  for (uint32_t t = 0; t < T; t += 3) {
    LM_HASH_LOAD(xc, t + 2); LM_HASH_CHAIN(xa, t);
    LM_HASH_LOAD(xa, t + 3); LM_HASH_CHAIN(xb, t + 1);
    LM_HASH_LOAD(xb, t + 4); LM_HASH_CHAIN(xc, t + 2);
  }
#undef LM_HASH_LOAD
#undef LM_HASH_CHAIN
  // the last partial KB: chunks of four stripes, each stripe under its own test
  {
    const uint32_t s0 = n_kb << 6;
#pragma unroll 1
    for (uint32_t c = 0; c < 16; c++) {
      const uint32_t s_ = s0 + 4 * c;
      const uint32_t st_ = s_ + (rl >> 2), stc_ = st_ < n_str ? st_ : (n_str ? n_str - 1 : 0u);
      const uint32_t x = ((const uint32_t*)p)[(size_t)4 * stc_ + a];
      const uint32_t m_ = x * P2;
      uint32_t nv = xx_round(v, m_);
      if (s_ < n_str) v = nv;
      nv = xx_round(v, lmw::row_down<4>(m_));
      if (s_ + 1 < n_str) v = nv;
      nv = xx_round(v, lmw::row_down<8>(m_));
      if (s_ + 2 < n_str) v = nv;
      nv = xx_round(v, lmw::row_down<12>(m_));
      if (s_ + 3 < n_str) v = nv;
    }
  }
  int g0 = (int)(lane & ~15u);
  uint32_t v1 = lmw::shfl(v, g0), v2 = lmw::shfl(v, g0 + 1), v3 = lmw::shfl(v, g0 + 2), v4 = lmw::shfl(v, g0 + 3);
  uint32_t h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
  h += (uint32_t)len;
  const uint8_t* q = p + ((uint64_t)n_str << 4);
  const uint8_t* end = p + len;
  while (q + 4 <= end) { h = rotl32(h + ld32le(q) * P3, 17) * P4; q += 4; }
  while (q < end) { h = rotl32(h + (*q) * P5, 11) * P1; q++; }
  h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
  if (have && rl == 0) d.blob_hash[b] = len >= 16 ? h : 0u;
}

// K1: one lane per blob — envelope, xxh32, block count.
LM_KERNEL void k_frame_count(Dev d) {
  uint32_t b = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (b >= d.n_blobs) return;
  const uint8_t* p = d.data + d.blob_off[b];  // blob starts are 16-byte aligned by the host packer
  uint64_t len = d.blob_len[b];
  int32_t st = ST_OK;
  uint32_t nblk = 0;
  if (len < 22) st = ST_DECODE_ERROR;
  else if (!(p[0] == 'l' && p[1] == 'o' && p[2] == 'r' && p[3] == 'o')) st = ST_DECODE_ERROR;
  else {
    uint32_t mode = ((uint32_t)p[20] << 8) | p[21];
    if (mode == 3) st = ST_UNSUPPORTED;        // FastSnapshot: outside the hot-path scope
    else if (mode != 4) st = ST_DECODE_ERROR;
    else {
      uint32_t expect = ld32le(p + 16);
      // large blobs were hashed by a wave each (k_hash_big_blobs); the others by this lane
      uint32_t h = len >= BIG_BLOB ? d.blob_hash[b] : xxh32_lane(p + 20, len - 20, 0x4f524f4cu);
      if (h != expect) st = ST_CHECKSUM_MISMATCH;
      else {
        Rd r = rd_make(p + 22, len - 22);
        while (r.p < r.end && !r.bad) {
          uint64_t bl = rd_uleb(r);
          if (bl == 0 || bl > rd_left(r)) { r.bad = true; break; }
          r.p += bl;
          nblk++;
        }
        if (r.bad) { st = ST_DECODE_ERROR; nblk = 0; }
      }
    }
  }
  d.blob_status[b] = st;
  d.blob_nblk[b] = nblk;
}

// K2a: one lane per blob — where every block of the blob begins (the frames are a chain: `uleb len + block`, fast_snapshot.rs:372-400).
// Only the chain is walked here; the blocks' descriptors are filled in parallel by k_block_desc (a 2.4 MB blob holds 400 blocks:
// parsed one after the other by this one lane they were 7 ms of a configs[2] batch).
LM_KERNEL void k_frame_fill(Dev d) {
  uint32_t b = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (b >= d.n_blobs) return;
  if (d.blob_status[b] != ST_OK) return;
  uint64_t base = d.blob_off[b];
  const uint8_t* p = d.data + base;
  uint64_t len = d.blob_len[b];
  Rd r = rd_make(p + 22, len - 22);
  uint32_t bi = d.blob_blk0[b];
  uint32_t nblk = d.blob_nblk[b];
  uint32_t doc = d.blob_doc[b];
  for (uint32_t k = 0; k < nblk; k++, bi++) {
    uint64_t bl = rd_uleb(r);
    BlockDesc* o = d.blk + bi;
    o->base = (uint64_t)(r.p - d.data);
    o->blob = b;
    o->doc = doc;
    o->pad = (uint32_t)bl;     // (the block's length, for k_block_desc; a frame is shorter than its blob, a blob shorter than 4 GiB)
    r.p += bl;                 // (k_frame_count checked every frame against the blob's end)
  }
}
// K2b: one lane per block — the postcard struct head and the section extents (block_encode.rs:94-119).
LM_KERNEL void k_block_desc(Dev d) {
  uint32_t bi = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (bi >= d.n_blocks) return;
  BlockDesc bd = d.blk[bi];
  const uint8_t* p0 = d.data + bd.base;
  Rd q = rd_make(p0, bd.pad);
  uint64_t cs = rd_uleb(q), cl = rd_uleb(q), ls = rd_uleb(q), ll = rd_uleb(q), nc = rd_uleb(q);
  bd.status = ST_OK;
  bd.flags = 0; bd.pad = 0;
  if (cs > 0x7fffffffull || cl > 0x7fffffffull || ls > 0xffffffffull || ll > 0xffffffffull || nc > 0x7fffffffull || nc == 0)
    bd.status = ST_DECODE_ERROR;
  if (cs + cl > MAX_COUNTER) bd.status = bd.status ? bd.status : ST_UNSUPPORTED;
  bd.counter_start = (uint32_t)cs; bd.counter_len = (uint32_t)cl;
  bd.lamport_start = (uint32_t)ls; bd.lamport_len = (uint32_t)ll; bd.n_changes = (uint32_t)nc;
  for (int s = 0; s < (int)SEC_N; s++) {
    Rd sec = rd_bytes(q);
    bd.sec_rel[s] = (uint32_t)(sec.p - p0);
    bd.sec_len[s] = (uint32_t)rd_left(sec);
  }
  if (q.bad) bd.status = ST_DECODE_ERROR;
  d.blk[bi] = bd;
}

LM_DEV Rd blk_sec(const Dev& d, const BlockDesc& bd, int s) {
  return rd_make(d.data + bd.base + bd.sec_rel[s], bd.sec_len[s]);
}

// K3a (round 6): is this a block of Map ops with scalar values only?  One lane per block: the container ids (all of kind Map), the
// value_type column (every value 8 = delete or 11 = a tagged LoroValue — whether that value is a scalar is the fused kernel's
// business), no delete-start ids.  blk_kind = bit 31 | op rows.
static constexpr uint32_t BK_MAPSIMPLE = 0x80000000u;
LM_KERNEL void k_block_kind(Dev d) {
  uint32_t bi = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (bi >= d.n_blocks) return;
  const BlockDesc bd = d.blk[bi];
  uint32_t out = 0;
  if (bd.status == ST_OK && bd.sec_len[SEC_DEL] == 0) {
    bool ok = true;
    Rd k = blk_sec(d, bd, SEC_CIDS);
    uint64_t ncid = k.p < k.end ? rd_uleb(k) : 0;
    if (ncid == 0 || ncid > 32) ok = false;
    for (uint64_t i = 0; i < ncid && ok; i++) {
      uint64_t fields = rd_uleb(k);
      (void)rd_u8(k);
      uint32_t kind = rd_u8(k);
      (void)rd_uleb(k); (void)rd_zigzag(k);
      if (fields != 4 || kind != CK_MAP) ok = false;
    }
    if (k.bad || k.p != k.end) ok = false;
    uint64_t nops = 0;
    if (ok) {
      Rd o = blk_sec(d, bd, SEC_OPS);
      uint64_t outer = rd_uleb(o), ncols = rd_uleb(o);
      if (outer != 1 || ncols != 4) ok = false;
      (void)rd_bytes(o); (void)rd_bytes(o);
      Rd c2 = rd_bytes(o);
      if (o.bad) ok = false;
      while (ok && c2.p < c2.end) {
        int64_t kk = rd_zigzag(c2);
        if (kk == 0 || c2.bad) { ok = false; break; }
        uint64_t n = kk > 0 ? 1u : (uint64_t)(-kk);
        if (n > rd_left(c2)) { ok = false; break; }
        for (uint64_t j = 0; j < n; j++) { uint32_t vt = rd_u8(c2) & 0x7f; if (vt != 8 && vt != 11) ok = false; }
        nops += kk > 0 ? (uint64_t)kk : n;
        if (nops > (1u << 24)) ok = false;
      }
    }
    if (ok && nops == bd.counter_len && nops > 0) out = BK_MAPSIMPLE | (uint32_t)nops;
  }
  d.blk_kind[bi] = out;
}
// … and is this a document of such blocks (one lane per document)?  Worth a workgroup of its own only with enough rows; a history of
// one change per write is left to the row tables (the fused kernel walks a block's changes one after the other).
LM_KERNEL void k_doc_kind(Dev d, uint8_t* doc_fused, uint32_t min_rows, uint32_t chg_ratio) {
  uint32_t doc = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (doc >= d.n_docs) return;
  uint32_t b0 = d.doc_blob[doc], b1 = d.doc_blob[doc + 1];
  uint32_t k0 = d.blob_blk0[b0], k1 = d.blob_blk0[b1];
  bool ok = k1 > k0;
  uint64_t rows = 0, chg = 0;
  for (uint32_t b = b0; b < b1 && ok; b++) ok = d.blob_status[b] == ST_OK;
  for (uint32_t k = k0; k < k1 && ok; k++) {
    uint32_t v = d.blk_kind[k];
    if (!(v & BK_MAPSIMPLE)) ok = false;
    rows += v & 0x7fffffffu; chg += d.blk[k].n_changes;
  }
  doc_fused[doc] = ok && rows >= min_rows && rows < (1u << 24) && chg * chg_ratio <= rows ? 1 : 0;
}

// K3: one lane per block — count the rows each table will receive.
LM_KERNEL void k_block_count(Dev d) {
  uint32_t bi = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (bi >= d.n_blocks) return;
  BlockDesc bd = d.blk[bi];
  uint32_t* c = d.bcnt + (uint64_t)bi * BCN;
  for (int i = 0; i < BCN; i++) c[i] = 0;
  if (bd.status != ST_OK) return;
  uint32_t N = bd.n_changes;
  bool bad = false;
  // header: peers, N-1 lens, BoolRle[N], AnyRle[N] dep counts
  Rd h = blk_sec(d, bd, SEC_HEADER);
  uint64_t np = rd_uleb(h);
  if (np == 0 || np > rd_left(h) / 8 || np > MAX_PEERS) bad = true;
  uint64_t ndep = 0;
  if (!bad) {
    rd_skip(h, np * 8);
    for (uint32_t i = 0; i + 1 < N && !h.bad; i++) (void)rd_uleb(h);
    BoolCur bc = bool_make(h);
    for (uint32_t i = 0; i < N && !bc.r.bad; i++) if (bool_next(bc)) ndep++;
    if (bc.rem != 0) bc.r.bad = true;
    RleCur dc = rle_make(bc.r);
    for (uint32_t i = 0; i < N && !dc.r.bad; i++) ndep += rle_next_uvar(dc);
    if (dc.rem != 0) dc.r.bad = true;
    if (dc.r.bad || ndep > (1u << 28)) bad = true;
  }
  // ops: count rows through the value_type column (raw-byte literals)
  uint64_t nops = 0, nmap = 0;
  {
    Rd o = blk_sec(d, bd, SEC_OPS);
    uint64_t outer = rd_uleb(o), ncols = rd_uleb(o);
    if (outer != 1 || ncols != 4) bad = true;
    Rd c0 = rd_bytes(o); (void)c0;
    Rd c1 = rd_bytes(o); (void)c1;
    Rd c2 = rd_bytes(o);
    if (o.bad) bad = true;
    if (!bad) { nops = rle_count_u8(c2); if (nops == ~0ull) bad = true; }
    // every op row covers at least one op id of the block (block_encode.rs:651-704 advances the counter by the row's len; the
    // writers never emit an empty op), so a value-type column that announces more rows than the block has ids — a run count of
    // 2^28 in two bytes — cannot decode to a block: DecodeError here, before any table is sized by it
    if (!bad && nops > (uint64_t)bd.counter_len) bad = true;
  }
  const bool fused = d.doc_fused && d.doc_fused[bd.doc];   // (lm_k_map_fused.h: no op rows, no key rows but the root containers' names)
  uint64_t nkeys = 0;
  if (!fused) {
    Rd k = blk_sec(d, bd, SEC_KEYS);
    while (k.p < k.end && !k.bad) { uint64_t l = rd_uleb(k); rd_skip(k, l); nkeys++; }
    if (k.bad) bad = true;
  }
  uint64_t ncid = 0;
  {
    Rd k = blk_sec(d, bd, SEC_CIDS);
    if (k.p < k.end) ncid = rd_uleb(k);
    if (k.bad || ncid > (1u << 20)) bad = true;
    if (fused && !bad) {   // one key row per ROOT container id (k_doc_tables reads the names through them)
      for (uint64_t i = 0; i < ncid; i++) { (void)rd_uleb(k); uint32_t is_root = rd_u8(k); (void)rd_u8(k); (void)rd_uleb(k); (void)rd_zigzag(k); nkeys += is_root ? 1u : 0u; }
    }
  }
  if (bad) { d.blk[bi].status = ST_DECODE_ERROR; return; }
  (void)nmap;
  if (!fused) {   // heads beyond the decoder's default LDS slot (Map blocks with hundreds of keys, blocks of thousands of changes): the host
      // launches the decoder a second time, with larger slots, for the groups that hold one (lm_pipeline.h)
    uint32_t span = (uint32_t)(bd.base & 15) + bd.sec_rel[SEC_VALUES];
    if (d.dec_stat && span > d.dec_slot) {
      lmw::atomic_add(&d.dec_stat[0], 1u); lmw::atomic_max32(&d.dec_stat[1], span);
      lmw::atomic_max32(&d.dec_stat[2], (uint32_t)((bd.base + bd.sec_rel[SEC_OPS]) & 15) + bd.sec_rel[SEC_VALUES] - bd.sec_rel[SEC_OPS]);   // … and of its op / delete-start columns alone
    }
  }
  c[BC_CHG] = N;
  c[BC_DEP] = (uint32_t)ndep;
  c[BC_OP] = fused ? 0u : (uint32_t)nops;
  c[BC_KEY] = (uint32_t)nkeys;
  c[BC_CID] = (uint32_t)ncid;
  c[BC_PEER] = (uint32_t)np;
  c[BC_MAPOP] = fused ? (uint32_t)nops : 0u;   // rows of a fused Map document (lm_k_map_fused.h): the capacity of its record table, handed out behind the op rows (k_doc_ranges)
  c[BC_ATOMS] = bd.counter_len;
}

// skip one nested LoroValue (docs/encoding.md §10.1); iterative with an explicit frame stack.
// `unsupported` is raised for shapes the device emitter does not render (a container below the accepted depth).  A child
// container (tag 9 + kind byte) is accepted down to nesting depth `cdepth`: 0 for a Map value, 1 for the items of a List
// insert; -1 nowhere.  Children of a kind outside Map / List / Text are accepted here: they render as null and flag the
// document DF_SOFT_UNSUPPORTED when met by the emitter (or when one of their ops is applied).
// (a scalar at the top level — what a Map set or a list of numbers carries — is stepped over right here: the frame machinery below
// is for lists, maps and child containers)
// corrupt values: the reference decodes EVERY value in full when it decodes the block — a nested map whose key index lies beyond
// the block's key table, a value tag nobody defined, a collection of more than 2^28 items are DecodeDataCorruptionError there
// whether or not the value ever reaches the state (value.rs:342-459).  The decoders' walk (KEYS = false) latches the reader (`bad`)
// on the last two — the block is rejected — and leaves key indices to k_remap, which walks the rows flagged OPF_NESTED a second
// time with KEYS = true and reports all three as VF_CORRUPT.
// (`vf`: bit 0 = a shape the device does not render, bit 1 = corrupt.  Measured with -Rpass-analysis=kernel-resource-usage: every
// extra write to a caller's flag inside this routine, inlined into the wave decoder's walker, costs that kernel 100-300 spilled
// scalars and ~20 % of its time — hence the template switch rather than a run-time one)
static constexpr uint32_t VF_UNSUPPORTED = 1u, VF_CORRUPT = 2u;
template <bool KEYS = false, class R> LM_DEV void skip_loro_value_fs(R& r, uint32_t& vf, int cdepth, uint32_t* f_cnt, uint32_t n_keys = 0xffffffffu);
template <class R> LM_DEV void skip_loro_value_top(R& r, uint32_t& vf, int cdepth, uint32_t* f_cnt, uint32_t tag_peek) {
  if (tag_peek > 6 || r.bad) { skip_loro_value_fs(r, vf, cdepth, f_cnt); return; }   // (a latched reader consumes nothing there)
  (void)rd_u8(r);
  if (tag_peek == 3) (void)rd_sleb(r);
  else if (tag_peek == 4) rd_skip(r, 8);
  else if (tag_peek >= 5) { uint64_t l = rd_uleb(r); rd_skip(r, l); }
}
template <bool KEYS, class R> LM_DEV void skip_loro_value_fs(R& r, uint32_t& vf, int cdepth, uint32_t* f_cnt, uint32_t n_keys) {   // f_cnt: 16 words of frame stack
  uint32_t f_map = 0;  // bit i: frame i is a map (each item is preceded by a key index)
  int sp = 0;
  uint32_t cnt = 1;
  bool in_map = false;
  for (uint32_t guard = 0; guard < (1u << 28); guard++) {
    while (cnt == 0) {
      if (sp == 0) return;
      sp--;
      cnt = f_cnt[sp];
      in_map = (f_map >> sp) & 1;
    }
    if (r.bad) return;
    cnt--;
    if (in_map) {
      uint64_t kidx = rd_uleb(r);
      if (KEYS) vf |= (kidx >= n_keys && !r.bad) ? VF_CORRUPT : 0u;
    }
    uint32_t tag = rd_u8(r);
    switch (tag) {
      case 0: case 1: case 2: break;
      case 3: (void)rd_sleb(r); break;
      case 4: rd_skip(r, 8); break;
      case 5: case 6: { uint64_t l = rd_uleb(r); rd_skip(r, l); break; }
      case 7: case 8: {
        uint64_t n = rd_uleb(r);
        if (KEYS) vf |= (n > (1u << 28) && !r.bad) ? VF_CORRUPT : 0u;
        if (n > (1u << 28) || sp >= 16) { r.bad = true; return; }
        f_cnt[sp] = cnt;
        f_map = (f_map & ~(1u << sp)) | ((in_map ? 1u : 0u) << sp);
        sp++;
        cnt = (uint32_t)n;
        in_map = tag == 8;
        break;
      }
      case 9: { (void)rd_u8(r); if (sp > cdepth) vf |= VF_UNSUPPORTED; break; }   // (any kind byte: ContainerType::Unknown, lib.rs:793-804)
      default: if (KEYS) vf |= r.bad ? 0u : VF_CORRUPT; r.bad = true; return;
    }
  }
  r.bad = true;
}
LM_DEV void skip_loro_value(Rd& r, uint32_t& vf, int cdepth = -1) {
  uint32_t f_cnt[16];
  skip_loro_value_fs(r, vf, cdepth, f_cnt);
}
LM_DEV void skip_loro_value_keys(Rd& r, uint32_t& vf, uint32_t n_keys) {
  uint32_t f_cnt[16];
  skip_loro_value_fs<true>(r, vf, -1, f_cnt, n_keys);
}
LM_DEV void skip_loro_value(Rd& r, bool& unsupported, int cdepth = -1) {   // (callers that only render: corruption shows as r.bad)
  uint32_t vf = 0;
  skip_loro_value(r, vf, cdepth);
  if (vf & VF_UNSUPPORTED) unsupported = true;
}

// (the lane decoder's verdicts: the first finding stays; the kernel-logic harness names the line, LM_EMU_TRACE)
#if defined(LM_EMU) && defined(LM_EMU_TRACE)
#define DEC_ST(code) do { if (!st) { if (getenv("LM_EMU_DEC")) fprintf(stderr, "lm emu: block verdict " #code " at %s:%d\n", __FILE__, __LINE__); st = (code); } } while (0)
#else
#define DEC_ST(code) do { st = st ? st : (code); } while (0)
#endif
// K4: one lane per block — full decode into the row tables (block-local indices; K6 remaps them).
// Per-block row statistics both decoders leave in the block's descriptor for k_dag_a (which used to read every op row of the
// document again just to count them — 10 GB per configs[2] batch): BlockDesc.flags = rows that compete in the LWW table (Map
// sets / deletes, MovableList moves / sets, rows of containers outside the device scope) | bit 31: the block holds a style
// anchor; BlockDesc.pad = elements its rows insert (the length of insert / anchor rows, one per move).
LM_DEV void kc_add(uint32_t& n_map, uint32_t& n_el, uint32_t& n_style, uint32_t k, uint32_t len) {
  n_map += (k == OK_MAP_SET || k == OK_MAP_DEL || k == OK_LIST_MOVE || k == OK_LIST_SET || k == OK_OTHER) ? 1u : 0u;
  n_el += (k == OK_TEXT_INS || k == OK_LIST_INS || k == OK_STYLE_START || k == OK_STYLE_END) ? len : (k == OK_LIST_MOVE ? 1u : 0u);
  n_style += (k == OK_STYLE_START || k == OK_STYLE_END) ? 1u : 0u;
}
LM_DEV uint32_t kc_pack(uint32_t n_map, uint32_t n_style) { return (n_map & 0x7fffffffu) | (n_style ? 0x80000000u : 0u); }

// EXACT (k_block_reclassify): the same sequential decode run once more over the blocks a decoder REJECTED with DecodeError, with the
// value walk that names corruption where it stands (an undefined value tag, a nested map key index beyond the block's key table, an
// oversized collection are DecodeDataCorruptionError in the reference, value.rs:342-459 — the hot decoders only latch their reader
// there and report the block as DecodeError at its end; a write to a flag inside their walker costs them ~20 %, see above).  Only the
// verdict (DecodeError / DataCorruption, whichever its sequential walk meets first) is taken from this pass: the rows it writes belong to
// a block whose document has failed.
static constexpr uint32_t DEC_RECLASS = 0xDEC0DE01u;   // BlockDesc.pad of a block a row decoder left with ST_DECODE_ERROR / ST_DATA_CORRUPTION
template <bool EXACT> LM_DEV void lane_skip_value(Rd& r, uint32_t& vf, int cdepth, uint32_t n_keys) {
  uint32_t f_cnt[16];
  if (EXACT) skip_loro_value_fs<true>(r, vf, cdepth, f_cnt, n_keys);
  else skip_loro_value_fs(r, vf, cdepth, f_cnt);
}
// HEAD (k_block_head): the blocks of the documents lm_k_map_fused.h decodes — header, change meta, container ids, the names of the root
// containers; no key rows, no op rows (the fused kernel reads the columns itself).  The other decoders leave those blocks alone.
template <bool EXACT, bool HEAD = false> LM_DEV void block_decode_lane(Dev d) {
  uint32_t bi = (uint32_t)(lmw::bid() * lmw::bdim() + lmw::tid());
  if (bi >= d.n_blocks) return;
  BlockDesc bd = d.blk[bi];
  if (EXACT ? ((bd.status != ST_DECODE_ERROR && bd.status != ST_DATA_CORRUPTION) || bd.pad != DEC_RECLASS) : (bd.status != ST_OK)) return;
  if (HEAD != (d.doc_fused && d.doc_fused[bd.doc])) return;
  const uint32_t* off = d.boff + (uint64_t)bi * BCN;
  const uint32_t* cnt = d.bcnt + (uint64_t)bi * BCN;
  uint32_t N = bd.n_changes;
  uint32_t chg0 = off[BC_CHG], dep0 = off[BC_DEP], op0 = off[BC_OP], key0 = off[BC_KEY], cid0 = off[BC_CID], peer0 = off[BC_PEER];
  uint32_t n_peers = cnt[BC_PEER], n_ops = cnt[BC_OP], n_keys = cnt[BC_KEY], n_cids = cnt[BC_CID];
  int32_t st = ST_OK;
  bool unsupported = false;
  uint32_t kc_map = 0, kc_el = 0, kc_style = 0;   // (kc_add)
  // ---- header
  Rd h = blk_sec(d, bd, SEC_HEADER);
  (void)rd_uleb(h);
  for (uint32_t i = 0; i < n_peers; i++) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)rd_u8(h) << (8 * k);
    d.peer_raw[peer0 + i] = v;
  }
  {
    // change lens → counters
    uint64_t known = 0;
    uint32_t ctr = bd.counter_start;
    for (uint32_t i = 0; i < N; i++) {
      uint64_t l;
      if (i + 1 < N) { l = rd_uleb(h); known += l; if (known > bd.counter_len) { st = ST_DECODE_ERROR; l = 0; } }
      else l = bd.counter_len - (known > bd.counter_len ? bd.counter_len : known);
      ChangeRow c;
      c.peer = 0; c.ctr = ctr; c.len = (uint32_t)l; c.dep0 = 0; c.n_dep = 0; c.op0 = 0; c.n_op = 0; c.blk = bi;
      d.chg[chg0 + i] = c;
      ctr += (uint32_t)l;
    }
    // dep_on_self BoolRle[N]  (kept in op0 until the op rows are assigned)
    BoolCur bc = bool_make(h);
    for (uint32_t i = 0; i < N; i++) d.chg[chg0 + i].op0 = bool_next(bc) ? 1u : 0u;
    if (bc.rem != 0) bc.r.bad = true;
    // other dep counts AnyRle<usize>[N]
    RleCur dc = rle_make(bc.r);
    uint32_t dcur = dep0;
    uint64_t others_total = 0;
    for (uint32_t i = 0; i < N; i++) {
      uint64_t others = rle_next_uvar(dc);
      ChangeRow c = d.chg[chg0 + i];
      uint32_t ds = c.op0;
      if (dcur + ds + others > dep0 + cnt[BC_DEP]) { st = ST_DECODE_ERROR; others = 0; ds = 0; }
      others_total += others;
      c.dep0 = dcur;
      c.n_dep = ds + (uint32_t)others;
      if (ds) {
        if (c.ctr == 0) st = ST_DECODE_ERROR;
        d.dep_peer[dcur] = 0;
        d.dep_ctr[dcur] = c.ctr ? c.ctr - 1 : 0;
      }
      dcur += c.n_dep;
      d.chg[chg0 + i] = c;
    }
    if (dc.rem != 0) dc.r.bad = true;
    if (dcur - dep0 != cnt[BC_DEP]) st = ST_DECODE_ERROR;
    // dep peer idx AnyRle<u32>[D]
    RleCur pc = rle_make(dc.r);
    uint64_t D = 0;
    for (uint32_t i = 0; i < N && others_total; i++) {   // (no dependency on another peer in the whole block: both columns are empty)
      ChangeRow c = d.chg[chg0 + i];
      for (uint32_t k = c.dep0 + c.op0; k < c.dep0 + c.n_dep; k++) {
        uint64_t pi = rle_next_uvar(pc);
        if (pi >= n_peers) { st = ST_DECODE_ERROR; pi = 0; }
        d.dep_peer[k] = (uint32_t)pi;
        D++;
      }
    }
    if (pc.rem != 0) pc.r.bad = true;
    // dep counters DeltaOfDelta[D]
    Rd hr = pc.r;
    DodCur dd = dod_make(hr);
    for (uint32_t i = 0; i < N && D; i++) {
      ChangeRow c = d.chg[chg0 + i];
      for (uint32_t k = c.dep0 + c.op0; k < c.dep0 + c.n_dep; k++) {
        int64_t v = dod_next(dd);
        if (v < 0 || v >= (int64_t)MAX_COUNTER) { st = st ? st : ST_DECODE_ERROR; v = 0; }
        d.dep_ctr[k] = (uint32_t)v;
      }
    }
    dod_finish(dd, hr, D);
    // wire lamports (DeltaOfDelta[N-1]) are validated for shape only: lamports are recomputed from deps on
    // import (outdated_encode_reordered.rs:61-62)
    DodCur ld = dod_make(hr);
    dod_skip(ld, N ? N - 1 : 0);
    dod_finish(ld, hr, N - 1);
    {   // the last change's lamport = lamport_start + lamport_len - its length, in u32 with checked arithmetic (block_meta_encode.rs:215-221):
        // the wire lamports are not used (recomputed from the dependencies on import), this verdict is
      const uint64_t kn_ = known > bd.counter_len ? bd.counter_len : known;
      const uint64_t lend = (uint64_t)bd.lamport_start + (uint64_t)bd.lamport_len, last_len = (uint64_t)bd.counter_len - kn_;
      if (lend > 0xFFFFFFFFull || lend < last_len) st = st ? st : ST_DECODE_ERROR;
    }
    if (h.bad || bc.r.bad || dc.r.bad || pc.r.bad || hr.bad) st = st ? st : ST_DECODE_ERROR;
    for (uint32_t i = 0; i < N; i++) d.chg[chg0 + i].op0 = 0;
  }
  // ---- change_meta: timestamps + message lengths, shape only (block_encode.rs:563-571)
  {
    Rd m = blk_sec(d, bd, SEC_META);
    DodCur td = dod_make(m);
    dod_skip(td, N);
    dod_finish(td, m, N);
    RleCur mc = rle_make(m);
    const uint64_t tot = rle_sum_uvar(mc, N);
    // (the reference maps EVERY failure of these two columns — a timestamp stream that does not decode, too few values, a run that
    // announces more than N — to DecodeDataCorruptionError (block_encode.rs:563-571: `.map_err(|_| LoroError::DecodeDataCorruptionError)`
    // on both decoders; only the HEADER columns of block_meta_encode.rs are DecodeError); lengths beyond the message bytes likewise)
    if (mc.rem != 0) mc.r.bad = true;
    if (mc.r.bad || tot > rd_left(mc.r)) DEC_ST(ST_DATA_CORRUPTION);
  }
  // ---- keys
  if (!HEAD) {
    Rd k = blk_sec(d, bd, SEC_KEYS);
    for (uint32_t i = 0; i < n_keys; i++) {
      uint64_t l = rd_uleb(k);
      d.key_off[key0 + i] = (uint64_t)(k.p - d.data);
      d.key_len[key0 + i] = (uint32_t)l;
      rd_skip(k, l);
    }
    if (k.bad) st = st ? st : ST_DECODE_ERROR;
  }
  uint32_t head_root = 0;   // HEAD: root container ids met so far = the block's next key row
  // ---- cids (arena.rs:39-105)
  {
    Rd k = blk_sec(d, bd, SEC_CIDS);
    if (n_cids) (void)rd_uleb(k);
    for (uint32_t i = 0; i < n_cids; i++) {
      uint64_t fields = rd_uleb(k);
      uint32_t is_root = rd_u8(k), kind = rd_u8(k);
      uint64_t pidx = rd_uleb(k);
      int64_t koc = rd_zigzag(k);
      if (fields != 4) st = st ? st : ST_DECODE_ERROR;
      uint32_t* w = d.cid_raw + (uint64_t)(cid0 + i) * 4;
      if (HEAD && is_root) {
        // the name: the koc-th key of the block, found by walking that far (a root's name is among the first keys); its key row is
        // numbered by the root ids of the block
        Rd kk = blk_sec(d, bd, SEC_KEYS);
        bool found = koc >= 0;
        uint64_t l = 0;
        for (int64_t q = 0; found && q <= koc; q++) { if (kk.p >= kk.end) { found = false; break; } l = rd_uleb(kk); if (q < koc) rd_skip(kk, l); if (kk.bad) found = false; }
        if (found && l > rd_left(kk)) found = false;
        if (!found || head_root >= n_keys) { DEC_ST(ST_DATA_CORRUPTION); d.key_off[key0 + (head_root < n_keys ? head_root : 0)] = 0; d.key_len[key0 + (head_root < n_keys ? head_root : 0)] = 0; koc = 0; }
        else { d.key_off[key0 + head_root] = (uint64_t)(kk.p - d.data); d.key_len[key0 + head_root] = (uint32_t)l; koc = head_root; }
        head_root++;
      }
      else if (is_root) { if (koc < 0 || (uint64_t)koc >= n_keys) { DEC_ST(ST_DATA_CORRUPTION); koc = 0; } }
      else { if (pidx >= n_peers) { DEC_ST(ST_DATA_CORRUPTION); pidx = 0; } if (koc < 0 || koc >= (int64_t)MAX_COUNTER) { st = st ? st : ST_UNSUPPORTED; koc = 0; } }
      w[0] = kind | (is_root ? 0x100u : 0u);
      w[1] = (uint32_t)pidx;
      w[2] = (uint32_t)koc;
      w[3] = bi;
      // (a kind beyond Counter is ContainerType::Unknown(kind), loro-common/src/lib.rs:793-804 — try_from_u8 never fails: the container is outside the device scope like Tree / Counter)
    }
    if (k.bad) st = st ? st : ST_DECODE_ERROR;
  }
  if (HEAD) {
    // the rows are the fused kernel's: every one competes in the LWW table, none inserts an element
    // (any finding: no verdict from here — k_block_count skipped this block's key table, so the row decoders, which own every error
    // code, may meet something else first: the document goes through them, DF_REDO)
    d.blk[bi].status = (st != ST_OK || unsupported) ? (int32_t)ST_MF_BAIL : (int32_t)ST_OK;
    d.blk[bi].flags = kc_pack(d.blk_kind[bi] & 0x7fffffffu, 0); d.blk[bi].pad = 0;
    return;
  }
  // ---- op rows
  {
    Rd o = blk_sec(d, bd, SEC_OPS);
    (void)rd_uleb(o); (void)rd_uleb(o);
    RleCur c_cont = rle_make(rd_bytes(o));
    RleCur c_prop = rle_make(rd_bytes(o));
    RleCur c_vt = rle_make(rd_bytes(o));
    RleCur c_len = rle_make(rd_bytes(o));
    Rd dsec = blk_sec(d, bd, SEC_DEL);
    bool has_del = dsec.p < dsec.end;
    RleCur d_peer = rle_make(dsec), d_ctr = rle_make(dsec), d_len = rle_make(dsec);
    if (has_del) {
      uint64_t outer = rd_uleb(dsec), ncols = rd_uleb(dsec);
      if (outer != 1 || ncols != 3) st = st ? st : ST_DECODE_ERROR;
      d_peer = rle_make(rd_bytes(dsec));
      d_ctr = rle_make(rd_bytes(dsec));
      d_len = rle_make(rd_bytes(dsec));
    }
    {
      // every column decodes, the op columns to one value per row, the delete-start columns to equally many (lm_dev_util.h rle_drain)
      bool colbad = false;
      { RleCur t = c_cont; uint32_t n = rle_drain(t, 2, n_ops); colbad |= t.r.bad || n != n_ops; }
      { RleCur t = c_prop; uint32_t n = rle_drain(t, 2, n_ops); colbad |= t.r.bad || n != n_ops; }
      { RleCur t = c_vt; uint32_t n = rle_drain(t, 0, n_ops); colbad |= t.r.bad || n != n_ops; }
      { RleCur t = c_len; uint32_t n = rle_drain(t, 1, n_ops); colbad |= t.r.bad || n != n_ops; }
      if (has_del) {
        RleCur t1 = d_peer, t2 = d_ctr, t3 = d_len;
        uint32_t n1 = rle_drain(t1, 2), n2 = rle_drain(t2, 2), n3 = rle_drain(t3, 2);
        colbad |= t1.r.bad || t2.r.bad || t3.r.bad || n1 != n2 || n1 != n3;
      }
      if (colbad) st = st ? st : ST_DECODE_ERROR;
    }
    Rd v = blk_sec(d, bd, SEC_VALUES);
    uint64_t counter = bd.counter_start;
    uint32_t change_index = 0;
    uint64_t next_boundary = N > 1 ? d.chg[chg0 + 1].ctr : (uint64_t)bd.counter_start + bd.counter_len;
    d.chg[chg0].op0 = op0;
    for (uint32_t row = 0; row < n_ops; row++) {
      int64_t ci = rle_next_delta(c_cont);
      int64_t prop = rle_next_delta(c_prop);
      uint32_t vt = rle_next_u8(c_vt) & 0x7f;
      uint64_t len = rle_next_uvar(c_len);
      if (ci < 0 || (uint64_t)ci >= n_cids) { DEC_ST(ST_DATA_CORRUPTION); ci = 0; }
      if (prop < INT32_MIN || prop > INT32_MAX) { st = st ? st : ST_DECODE_ERROR; prop = 0; }
      uint32_t ckind = n_cids ? (d.cid_raw[(uint64_t)(cid0 + (uint32_t)ci) * 4] & 0xff) : 0xff;
      OpRow r;
      r.cidx_kind = (uint32_t)ci;  // block-local until K6
      r.prop = (int32_t)prop;
      r.len = (uint32_t)len;
      r.ctr = (uint32_t)counter;
      r.a0 = 0; r.a1 = 0; r.a2 = 0;
      r.chg = chg0 + change_index;
      uint64_t val_at = (uint64_t)(v.p - d.data);
      uint32_t kind = OK_OTHER;
      uint32_t mark_len = 0;
      uint64_t mv_from = 0, mv_peer = 0, mv_lam = 0;
      uint32_t vfl = 0;        // (skip_loro_value: VF_UNSUPPORTED | VF_CORRUPT — an undefined value tag, an oversized collection)
      bool nested = false;     // the value is a list / map, or a payload that may hold one: OPF_NESTED (k_remap checks its key indices)
      bool is_list_value = false;
      // value payload (docs/encoding.md §10)
      switch (vt) {
        case 0: case 1: case 2: case 8: case 9: break;
        case 3: (void)rd_sleb(v); break;
        case 4: rd_skip(v, 8); break;
        case 5: case 6: { uint64_t l = rd_uleb(v); rd_skip(v, l); break; }
        case 7: (void)rd_uleb(v); break;
        case 10: (void)rd_sleb(v); break;
        case 11: {
          // peek the top-level tag to know whether it is a list (List insert) before skipping
          is_list_value = v.p < v.end && *v.p == 7;
          nested = v.p < v.end && (*v.p == 7 || *v.p == 8);
          if (is_list_value) {
            Rd t = v;
            (void)rd_u8(t);
            r.a0 = (uint32_t)rd_uleb(t);
          }
          // (values of containers outside the device scope are never rendered: any shape is accepted)
          lane_skip_value<EXACT>(v, vfl, ckind == CK_MAP ? 0 : (is_list_value && (ckind == CK_LIST || ckind == CK_MOVABLE) ? 1 : (ckind > CK_TEXT && ckind != CK_MOVABLE ? 16 : -1)), n_keys);
          break;
        }
        case 12: {
          (void)rd_u8(v);
          mark_len = (uint32_t)rd_uleb(v);
          uint64_t key_idx = rd_uleb(v);
          if (key_idx >= n_keys) DEC_ST(ST_DATA_CORRUPTION);
          uint32_t u = 0;
          lane_skip_value<EXACT>(v, u, -1, n_keys);
          vfl |= u & VF_CORRUPT;
          nested = true;
          break;
        }
        case 13: { (void)rd_uleb(v); uint32_t isn = rd_u8(v); (void)rd_uleb(v); if (!isn) (void)rd_uleb(v); break; }
        case 14: mv_from = rd_uleb(v); mv_peer = rd_uleb(v); mv_lam = rd_uleb(v); break;   // ListMove: source position, element peer idx, element lamport
        case 15: {   // ListSet: element peer idx, element lamport, then the nested value (op_val points at it)
          mv_peer = rd_uleb(v); mv_lam = rd_uleb(v);
          val_at = (uint64_t)(v.p - d.data);
          if (ckind == CK_MOVABLE) lane_skip_value<EXACT>(v, vfl, 0, n_keys);
          else { uint32_t u = 0; lane_skip_value<EXACT>(v, u, -1, n_keys); vfl |= u & VF_CORRUPT; }
          nested = true;
          break;
        }
        case 16: {
          (void)rd_uleb(v); (void)rd_uleb(v); (void)rd_uleb(v);
          uint32_t isn = rd_u8(v);
          if (!isn) { (void)rd_uleb(v); (void)rd_uleb(v); }
          break;
        }
        default: { uint64_t l = rd_uleb(v); rd_skip(v, l); break; }
      }
      if (vfl & VF_UNSUPPORTED) unsupported = true;
      if (vfl & VF_CORRUPT) DEC_ST(ST_DATA_CORRUPTION);
      // (EXACT: a value that runs out of input ends the reference's decode at THIS row with DecodeError; the hot decoders go on with
      // a latched reader — which hands out zeros — and may note a data-corruption finding on a later row in front of their
      // end-of-block DecodeError)
      if (EXACT && v.bad) DEC_ST(ST_DECODE_ERROR);
      // decode_op mapping (outdated_encode_reordered.rs:215-476)
      bool take_del = false;
      if (ckind == CK_TEXT) {
        if (vt == 5) kind = OK_TEXT_INS;
        else if (vt == 9) { kind = OK_DEL; take_del = true; }
        else if (vt == 12) { kind = OK_STYLE_START; r.a0 = mark_len; }
        else if (vt == 0) kind = OK_STYLE_END;
        else DEC_ST(ST_DATA_CORRUPTION);
      } else if (ckind == CK_MAP) {
        if (prop < 0 || (uint64_t)prop >= n_keys) DEC_ST(ST_DATA_CORRUPTION);
        if (vt == 8) kind = OK_MAP_DEL;
        else if (vt == 11) kind = OK_MAP_SET;
        else DEC_ST(ST_DATA_CORRUPTION);
      } else if (ckind == CK_LIST) {
        if (vt == 11) { if (is_list_value) kind = OK_LIST_INS; else DEC_ST(ST_DATA_CORRUPTION); }
        else if (vt == 9) { kind = OK_DEL; take_del = true; }
        else DEC_ST(ST_DATA_CORRUPTION);
      } else if (ckind == CK_MOVABLE) {   // outdated_encode_reordered.rs:388-459
        if (vt == 11) { if (is_list_value) kind = OK_LIST_INS; else DEC_ST(ST_DATA_CORRUPTION); }
        else if (vt == 9) { kind = OK_DEL; take_del = true; }
        else if (vt == 14 || vt == 15) {
          kind = vt == 14 ? OK_LIST_MOVE : OK_LIST_SET;
          if (mv_peer >= n_peers || mv_lam > 0xFFFFFFFFull || mv_from > 0x7FFFFFFFull || prop < 0 || len != 1) { DEC_ST(ST_DATA_CORRUPTION); mv_peer = 0; }
          r.a0 = (uint32_t)mv_peer; r.a1 = (uint32_t)mv_lam; r.a2 = (int32_t)(uint32_t)mv_from;
        } else DEC_ST(ST_DATA_CORRUPTION);
      }
      if (take_del) {
        if (!has_del) DEC_ST(ST_DATA_CORRUPTION);
        else {
          int64_t dp = rle_next_delta(d_peer), dctr = rle_next_delta(d_ctr), dl = rle_next_delta(d_len);
          if (dp < 0 || (uint64_t)dp >= n_peers) { DEC_ST(ST_DATA_CORRUPTION); dp = 0; }
          if (dl == 0 || dl > (int64_t)MAX_COUNTER || dl < -(int64_t)MAX_COUNTER) { DEC_ST(ST_DATA_CORRUPTION); dl = 1; }
          if (dctr < 0 || dctr >= (int64_t)MAX_COUNTER) { DEC_ST(ST_DATA_CORRUPTION); dctr = 0; }
          r.a0 = (uint32_t)dp; r.a1 = (uint32_t)dctr; r.a2 = (int32_t)dl;
          if (d_peer.r.bad || d_ctr.r.bad || d_len.r.bad) DEC_ST(ST_DATA_CORRUPTION);
        }
      }
      r.cidx_kind |= (kind << 16) | ((nested && (vt != 12 || kind == OK_STYLE_START)) ? OPF_NESTED : 0u);
      kc_add(kc_map, kc_el, kc_style, kind, (uint32_t)len);
      d.op[op0 + row] = r;
      d.op_val[op0 + row] = val_at;
      d.op_blk[op0 + row] = bi;
      counter += len;
      if (counter > MAX_COUNTER) { st = st ? st : ST_UNSUPPORTED; counter = MAX_COUNTER; }
      if (change_index >= N) { DEC_ST(ST_DATA_CORRUPTION); change_index = N - 1; }
      d.chg[chg0 + change_index].n_op++;
      if (counter > next_boundary && change_index + 1 < N) DEC_ST(ST_DATA_CORRUPTION);   // an op crosses a change boundary (docs/encoding.md §10.6)
      if (counter >= next_boundary && change_index + 1 < N) {
        change_index++;
        d.chg[chg0 + change_index].op0 = op0 + row + 1;
        next_boundary = change_index + 1 < N ? d.chg[chg0 + change_index + 1].ctr : (uint64_t)bd.counter_start + bd.counter_len;
      }
    }
    // changes that received no rows still need a valid op0
    for (uint32_t i = 1; i < N; i++) if (d.chg[chg0 + i].n_op == 0) d.chg[chg0 + i].op0 = op0 + n_ops;
    if (c_cont.r.bad || c_prop.r.bad || c_vt.r.bad || c_len.r.bad || v.bad) st = st ? st : ST_DECODE_ERROR;
    if (counter != (uint64_t)bd.counter_start + bd.counter_len) DEC_ST(ST_DATA_CORRUPTION);
  }
  if (EXACT) { if (st == ST_DATA_CORRUPTION || st == ST_DECODE_ERROR) d.blk[bi].status = st; return; }
  if (st == ST_OK && unsupported) st = ST_UNSUPPORTED;
  d.blk[bi].status = st;
  d.blk[bi].flags = kc_pack(kc_map, kc_style); d.blk[bi].pad = (st == ST_DECODE_ERROR || st == ST_DATA_CORRUPTION) ? DEC_RECLASS : kc_el;
}
LM_KERNEL void k_block_decode(Dev d) { block_decode_lane<false>(d); }
LM_KERNEL void k_block_head(Dev d) { block_decode_lane<false, true>(d); }
LM_KERNEL void k_block_reclassify(Dev d) { block_decode_lane<true>(d); }

}  // namespace lm

#include "lm_k_decode_wave.h"
