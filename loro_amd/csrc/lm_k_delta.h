// Text / List deltas between two versions (include/loro_merge.h lm_delta): what LoroDoc::diff(a, b) and the TextDelta / ListDiffItem
// events of subscribe tell a subscriber, answered on the device from the trackers and op rows the last run left — kernels of their
// own behind lm_run, like k_richtext and k_cursor: they read tracker memory (leaves, directory, status words, cp[] / tb[]) and the
// decoded op rows, and write only their own scratch, slabs and result rows.  The first part of this file is what lm_delta shares with
// lm_delta_map (lm_k_delta_map.h) and lm_delta_movable (lm_k_delta_movable.h): the query and result rows, the prologue of the *_mark
// kernels, bitmap marking, winner words, the walk over every element of a container, the run cutter and the result row.
//
// A = the version the subscriber has (the query's from_vv), V = the version the run rendered.  The definition is by ID SETS, so it
// does not depend on how the tracker got where it stands and A may be a version the tracker never stood at:
//   an element (p, c) is in A  iff  c < A[p] and no delete atom whose OWN id lies in A targets it;
//   it is in V                 iff  it is visible at the rendered version (the status word, as k_cursor / k_emit_text test it).
// The tracker keeps every element, tombstones included, in sequence order, and that order does not depend on the version: one walk
// over a container's leaves classifies every element as K (in both), I (in V only), D (in A only) or neither, and
//   a maximal run of K                          ->  {"retain":n}
//   the I and D between two K runs, interleaved ->  one {"insert":…} with all I in sequence order, then one {"delete":n}
// a trailing retain is dropped, a container whose delta is empty is left out.  Style anchors are never elements of a delta.
//
// k_delta_mark  lane = op row, grid over (query x 64-row chunks of the document's rows): the atoms of every delete row of a Text /
//               List container whose id lies below the bound — a version may cut a row — set their targets' bits in two bitmaps per
//               query indexed by element slot (elem_base[peer] + counter): deleted-in-A and deleted-in-V.  Rows of containers of
//               other kinds whose id lies in V \ A raise the query's other_changed.
// k_delta       one wave per query; per Text / List container every element in sequence order (dl_walk_all), classes by ballots.
//               SELF-CHECK: "in V by status" must equal "c < V[p] and bit V clear" for every element — a mismatch (a delete applied
//               by position, a damaged document, anything not thought of) gives the query LM_UNSUPPORTED: the right value or a
//               refusal, never a guess.  Class runs are coalesced across chunk and leaf boundaries through a wave-uniform carry (the
//               retain count, whether a gap / an insert is open, the pending delete count).  Text inserts are escaped and stored by
//               all lanes at once (cp_bytes + sink_lanes: the emitter's escapes, lengths by a DPP prefix scan), List values go through
//               the emitter's value sink one after the other.  Output goes into optimistic per-query slabs; the kernel never writes
//               beyond a slab and always reports the exact size (Engine::delta_run launches a second time at exact sizes when one
//               overflowed).
// k_delta_pack  one wave per query: the written bytes out of the slabs into one dense buffer — only that buffer goes to the host.
#pragma once
#include "lm_k_cursor.h"

namespace lm {

// ---- shared by the three delta calls
struct DlQuery {        // one per query, filled by Engine::delta_run
  uint32_t doc;
  uint32_t n_bnd;       // peers of the document: A[p] = bnd[bnd0 + p], V[p] = bnd[bnd0 + n_bnd + p] (decoded by the host)
  uint64_t bnd0;
  uint64_t scr0;        // the query's scratch, cleared by the host: an even index of 32-BIT WORDS into the call's scratch buffer.  First
                        // the 64-bit winner words winV[cap], winA[cap] (dl_win), then the bitmaps gone-at-A[n_words], gone-at-V[n_words]
                        // (dl_bits); a call that has no use for one of the two leaves cap / n_words 0
  uint32_t cap;         // slots of the document's table (ht_cap)
  uint32_t n_words;     // 32-bit words of one bitmap
  uint32_t n_bits;      // element slots a bitmap covers
  uint32_t row_blk0;    // the *_mark kernels: first workgroup of this query (ascending over the queries)
};
struct DlRes {          // one per query; cleared by the host in front of the *_mark kernel
  int32_t status;
  uint32_t other_changed;
  uint32_t len;         // exact size of the query's JSON
  uint32_t cnt;         // members written (the host orders them)
};
LM_DEV unsigned long long* dl_win(uint32_t* scr, const DlQuery& Q) { return (unsigned long long*)(scr + Q.scr0); }
LM_DEV uint32_t* dl_bits(uint32_t* scr, const DlQuery& Q) { return scr + Q.scr0 + 4ull * Q.cap; }
LM_DEV void dl_refuse(DlRes* res, uint32_t q) { (void)lmw::atomic_max32((uint32_t*)&res[q].status, (uint32_t)ST_UNSUPPORTED); }

// the prologue of the *_mark kernels (lane = op row, grid over query x 64-row chunks): the last query whose first workgroup is at
// or in front of this one (a query without rows owns none), its document, this lane's row and what every caller asks of it.  false:
// no row for this lane.  (The rows of a document that failed are not looked at: the host asks nothing about one, delta_bounds.)
struct DlRow {
  uint32_t q, i;        // the query; the row inside the document
  uint32_t kind, cidx, peer, bA, bV, ck;   // op kind, container, the change's peer index and its bounds at A / V, container kind
  DlQuery Q;
  DocMeta m;
  OpRow r;
  ChangeRow ch;
};
LM_DEV bool dl_mark_row(const Dev& d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, DlRow& x) {
  const uint32_t b = (uint32_t)lmw::bid();
  uint32_t lo = 0, hi = nq;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (qs[mid].row_blk0 <= b) lo = mid; else hi = mid; }
  x.q = lo;
  x.Q = qs[lo];
  x.m = d.doc[x.Q.doc];
  x.i = (b - x.Q.row_blk0) * 64 + (uint32_t)lmw::lane();
  if (x.i >= x.m.n_op || status_fatal(x.m.status)) return false;
  x.r = d.op[x.m.op0 + x.i];
  x.kind = (x.r.cidx_kind >> 16) & 0xff; x.cidx = x.r.cidx_kind & 0xffff;
  x.ch = d.chg[x.r.chg];
  x.peer = x.ch.peer;
  if ((x.cidx >= x.m.n_cont) | (x.peer >= x.Q.n_bnd)) return false;   // (one branch: with two the row's loads wait for the first one)
  x.bA = bnd[x.Q.bnd0 + x.peer]; x.bV = bnd[x.Q.bnd0 + x.Q.n_bnd + x.peer];
  x.ck = d.cont[x.m.cid0 + x.cidx].kind_root & 0xff;
  return true;
}
// a row with an id in V \ A (a container of a kind the call does not render raises bit 0 of other_changed with it)
LM_DEV bool dl_other_changed(const OpRow& r, uint32_t bA, uint32_t bV) { return r.ctr < bV && (uint64_t)r.ctr + (r.len ? r.len : 1u) > bA; }

// the element slots [g0, g1), g0 < g1, into a bitmap: word-wise atomic_or, one mask per touched word.  false, and nothing set: the
// range ends beyond the bitmap
LM_DEV bool dl_mark_range(uint32_t* bits, uint32_t n_bits, uint64_t g0, uint64_t g1) {
  if (g1 > n_bits) return false;
  const uint32_t w0 = (uint32_t)(g0 >> 5), w1 = (uint32_t)((g1 - 1) >> 5);
  for (uint32_t k = w0; k <= w1; k++) {
    const uint32_t lo_b = k == w0 ? (uint32_t)(g0 & 31) : 0u, hi_b = k == w1 ? (uint32_t)((g1 - 1) & 31) + 1u : 32u;
    const uint32_t mask = (hi_b == 32 ? 0xFFFFFFFFu : (1u << hi_b) - 1u) & ~((1u << lo_b) - 1u);
    (void)lmw::atomic_or(bits + k, mask);
  }
  return true;
}
// the delete row x.r: the targets of its atoms with ids below A into gone-at-A, below V into gone-at-V (dl_bits)
LM_DEV void dl_mark_delete(const Dev& d, const DlRow& x, uint32_t* bits, DlRes* res) {
  const OpRow& r = x.r;
  if (r.a0 >= x.Q.n_bnd) return;
  const uint32_t Ln = (uint32_t)(r.a2 < 0 ? -r.a2 : r.a2);
  const uint32_t eb = d.elem_base[x.m.praw0 + r.a0];
  for (int pass = 0; pass < 2; pass++) {
    const uint32_t bound = pass ? x.bV : x.bA;
    if (bound <= r.ctr) continue;
    uint32_t nb = bound - r.ctr;                      // the row's atoms [0, nb) have ids below the bound
    if (nb > r.len) nb = r.len;
    if (nb > Ln) nb = Ln;
    if (!nb) continue;
    const uint64_t g0 = (uint64_t)eb + r.a1 + (r.a2 > 0 ? 0u : Ln - nb);   // (lm_k_integrate_span.h: a backspace run targets its range back to front)
    if (!dl_mark_range(bits + (pass ? x.Q.n_words : 0u), x.Q.n_bits, g0, g0 + nb)) dl_refuse(res, x.q);
  }
}

// the packed word the table builders (k_map_lww, k_mlist_post) keep per slot, for the write row x.r: (lamport, peer index, row) + 1.
// 0: there is no such word — no table, not the table the host sized the scratch for, a row or a peer index beyond its field
LM_DEV unsigned long long dl_win_word(const Dev& d, const DlRow& x) {
  if (x.Q.cap == 0 || x.Q.cap != d.ht_cap[x.Q.doc] || x.i >= (1u << 24) || x.peer >= 256u) return 0;
  return (((unsigned long long)(d.chg_lamport[x.r.chg] + (x.r.ctr - x.ch.ctr)) << 32) | ((unsigned long long)x.peer << 24) | x.i) + 1;
}
LM_DEV uint32_t dl_win_row(unsigned long long w) { return (uint32_t)((w - 1) & 0xffffffu); }   // the row of a packed word, w != 0
// raise the winner at V (wV = winV + slot) and, for a row below A, the winner at A `cap` words behind it; a plain load first
// (k_map_lww: a row that is already beaten needs no atomic)
LM_DEV void dl_win_raise(unsigned long long* wV, uint32_t cap, unsigned long long v, bool below_A) {
  if (*wV < v) (void)lmw::atomic_max64(wV, v);
  if (below_A && wV[cap] < v) (void)lmw::atomic_max64(wV + cap, v);
}

// LoroValue equality of two plain values (loro-common/src/value.rs:29-44), one pair per lane.  0 = differ, 1 = equal, 2 = not decided
// here (two nested List values or two nested Map values), 3 = the bytes do not parse
LM_DEV uint32_t md_value_eq(const uint8_t* pa, const uint8_t* ea, const uint8_t* pb, const uint8_t* eb) {
  if (pa >= ea || pb >= eb) return 3;
  Rd a = rd_make(pa, (uint64_t)(ea - pa)), b = rd_make(pb, (uint64_t)(eb - pb));
  const uint32_t ta = rd_u8(a), tb = rd_u8(b);
  if (ta > 9 || tb > 9) return 3;
  if (ta != tb) return 0;                         // another kind (I64 3 against F64 3.0), true against false
  if (ta <= 2) return 1;
  if (ta == 3) { const int64_t x = rd_sleb(a), y = rd_sleb(b); return (a.bad || b.bad) ? 3u : (x == y ? 1u : 0u); }
  if (ta == 4) {                                  // a == b || (a.is_nan() && b.is_nan()): 0.0 equals -0.0
    uint64_t x = 0, y = 0;
    for (int k = 0; k < 8; k++) { x = (x << 8) | rd_u8(a); y = (y << 8) | rd_u8(b); }
    if (a.bad || b.bad) return 3;
    const uint64_t ax = x & 0x7fffffffffffffffull, ay = y & 0x7fffffffffffffffull, inf = 0x7ff0000000000000ull;
    if (ax > inf || ay > inf) return (ax > inf && ay > inf) ? 1u : 0u;
    if (ax == 0 && ay == 0) return 1;
    return x == y ? 1u : 0u;
  }
  if (ta == 5 || ta == 6) {
    const uint64_t la = rd_uleb(a), lb = rd_uleb(b);
    if (a.bad || b.bad || la > rd_left(a) || lb > rd_left(b)) return 3;
    if (la != lb) return 0;
    return bytes_eq(a.p, b.p, (uint32_t)la) ? 1u : 0u;
  }
  if (ta == 9) return 0;                          // a child container is named by its creating op: two ops, two ContainerIDs
  return 2;
}

// a value that is a child container (type byte 9, then the child's kind) is rendered as LoroValue::Container — the ContainerID of the
// op (eid_peer, eid_ctr) that created it — never as its content: rd_child tells, sink_child_cid writes
LM_DEV bool rd_child(Rd& r, uint32_t& child) {
  if (!(r.p < r.end && *r.p == 9)) return false;
  (void)rd_u8(r);
  child = rd_u8(r);
  return true;
}
LM_DEV void sink_child_cid(Sink& s, const Dev& d, const DocMeta& m, uint32_t eid_peer, uint32_t eid_ctr, uint32_t child, int32_t& err) {
  sink_lit(s, "\"\xF0\x9F\xA6\x9C:cid:", 10);
  sink_i64(s, (int64_t)eid_ctr);
  sink_byte(s, '@');
  sink_u64(s, eid_peer < m.n_peers ? d.peer_uniq[m.praw0 + eid_peer] : 0ull);
  if (child == CK_MAP) sink_lit(s, ":Map\"", 5);
  else if (child == CK_LIST) sink_lit(s, ":List\"", 6);
  else if (child == CK_TEXT) sink_lit(s, ":Text\"", 6);
  else if (child == CK_TREE) sink_lit(s, ":Tree\"", 6);
  else if (child == CK_MOVABLE) sink_lit(s, ":MovableList\"", 13);
  else if (child == CK_COUNTER) sink_lit(s, ":Counter\"", 9);
  else err = ST_UNSUPPORTED;
}

LM_DEV Sink dl_sink(uint8_t* out, const uint64_t* out_off, uint32_t q) {   // the query's slab
  Sink s;
  s.out = out + out_off[q];
  s.pos = 0;
  s.cap = out_off[q + 1] - out_off[q];
  return s;
}
// the result row.  (s_pos > the slab: the host sees the size and launches again with room for it; a size the row cannot hold is refused)
LM_DEV void dl_finish(DlRes* res, uint32_t q, int32_t err, uint64_t s_pos, uint32_t n_listed, uint32_t undecided) {
  if (s_pos > 0xfffffff0ull && !err) err = ST_UNSUPPORTED;
  undecided = lmw::any(undecided != 0) ? 2u : 0u;
  if (lmw::lane() == 0) {
    res[q].status = err ? err : (int32_t)ST_OK;
    res[q].len = err ? 0u : (uint32_t)s_pos;
    res[q].cnt = n_listed;
    if (!err && undecided) res[q].other_changed |= undecided;
  }
}

// ---- shared by the two kernels that walk the trackers (k_delta, k_mldelta)
struct DlLds {
  uint32_t eb[MAX_PEERS], bA[MAX_PEERS], bV[MAX_PEERS];   // per peer index: elem_base, A, V
  uint32_t inc[64];     // dl_walk_all, a span leaf: inclusive prefix of the items' lengths,
  uint32_t g0[64];      // … element slot of the item's first element, minus its exclusive prefix
  uint32_t i0[64];      // … its id, minus the same
  uint32_t st[64];      // … and its status word
};
struct DlDoc {
  uint32_t P, vis_mask;   // peers with a bound; the status bits that hide an element at the rendered version (k_cursor / k_emit_text)
  uint64_t elem0, data0, end;   // the document's element slots; its first byte; values are bounded by the end of its last blob (k_emit_any)
};
LM_DEV DlDoc dl_open(const Dev& d, const DlQuery& Q, const DocMeta& m, const uint32_t* bnd, DlLds& L) {
  DlDoc D;
  const uint32_t doc = Q.doc;
  D.elem0 = ((uint64_t)m.elem0_hi << 32) | m.elem0_lo;
  const bool at_version = d.res_vis && d.front_off[doc + 1] > d.front_off[doc] && !(m.flags & DF_FRONT_ERR);
  D.vis_mask = at_version ? (ST_FUT | ST_DELMASK) : ST_EVER;
  D.P = m.n_peers < Q.n_bnd ? m.n_peers : Q.n_bnd;
  D.data0 = d.blob_off[d.doc_blob[doc]];
  D.end = 0;
  if (d.doc_blob[doc + 1] > d.doc_blob[doc]) D.end = d.blob_off[d.doc_blob[doc + 1] - 1] + d.blob_len[d.doc_blob[doc + 1] - 1];
  for (uint32_t p = (uint32_t)lmw::lane(); p < MAX_PEERS; p += 64) {
    L.eb[p] = p < D.P ? d.elem_base[m.praw0 + p] : 0u;
    L.bA[p] = p < D.P ? bnd[Q.bnd0 + p] : 0u;
    L.bV[p] = p < D.P ? bnd[Q.bnd0 + Q.n_bnd + p] : 0u;
  }
  lmw::block_sync();
  return D;
}

// every element of a sequence container, tombstones included, in sequence order, 64 per step: f(has, pid, g, st) — the element's id,
// its slot inside the document (0 for a peer index >= P) and its status word — is called by all lanes together, lane order is sequence
// order; f returns false (wave-uniform) to end the walk.  Both tracker layouts; a span leaf is flattened 64 elements at a time.  (k_cursor's
// walk: the record of the next leaf and the directory entry behind it are requested before this leaf's elements are handled.)
template <class F>
LM_DEV void dl_walk_all(const Dev& d, const DocMeta& m, uint32_t cidx, uint32_t P, DlLds& L, F&& f) {
  const int lane = lmw::lane();
  const bool span = d.span != 0;
  const uint32_t rec_words = span ? SP_REC : 256u, st_at = span ? 256u : 192u;
  const uint32_t r0 = d.cont_root0[m.cid0 + cidx], nr = d.cont_nroot[m.cid0 + cidx];
  const uint32_t* dirp = d.dir_out + m.leaf0 + r0;
  uint32_t de1 = nr > 0 ? dirp[0] : 0u, de2 = nr > 1 ? dirp[1] : 0u;
  uint32_t p_id = NONE, p_ln = 1, p_st = ST_EVER;
  if (nr > 0 && (uint32_t)lane < de_n(de1)) {
    const uint32_t* rec = d.it + (uint64_t)(m.leaf0 + de_leaf(de1)) * rec_words;
    p_id = rec[lane]; p_st = rec[st_at + lane]; if (span) p_ln = rec[64 + lane];
  }
  for (uint32_t ri = 0; ri < nr; ri++) {
    const uint32_t id0 = p_id, ln = p_ln, st0 = p_st;
    de1 = de2;
    de2 = ri + 2 < nr ? dirp[ri + 2] : 0u;
    p_id = NONE; p_ln = 1; p_st = ST_EVER;
    if (ri + 1 < nr && (uint32_t)lane < de_n(de1)) {
      const uint32_t* rec = d.it + (uint64_t)(m.leaf0 + de_leaf(de1)) * rec_words;
      p_id = rec[lane]; p_st = rec[st_at + lane]; if (span) p_ln = rec[64 + lane];
    }
    const bool in = id0 != NONE;
    uint32_t total = 64;
    if (span) {
      const uint32_t al = in ? ln : 0u;
      const uint32_t inc = lmw::scan_incl_add(al);
      total = lmw::bcast(inc, 63);
      lmw::block_sync();
      L.inc[lane] = inc;
      L.g0[lane] = al && pid_peer(id0) < P ? L.eb[pid_peer(id0)] + pid_ctr(id0) - (inc - al) : 0u;
      L.i0[lane] = al ? id0 - (inc - al) : 0u;
      L.st[lane] = st0;
      lmw::block_sync();
    } else if (!lmw::any(in)) continue;
    for (uint32_t e0 = 0; e0 < total; e0 += 64) {
      bool has;
      uint32_t pid = NONE, g = 0, st = ST_EVER;
      if (span) {
        const uint32_t e = e0 + (uint32_t)lane;
        has = e < total;
        if (has) {
          uint32_t lo = 0, hi = 63;
          while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (L.inc[mid] > e) hi = mid; else lo = mid + 1; }
          g = L.g0[lo] + e; pid = L.i0[lo] + e; st = L.st[lo];
        }
      } else {
        has = in; pid = id0; st = st0;
        if (has && pid_peer(id0) < P) g = L.eb[pid_peer(id0)] + pid_ctr(id0);
      }
      if (!f(has, pid, g, st)) return;
    }
  }
}

// a 64-lane chunk's K / I / D ballots cut into alternating segments in lane order — a run of K, or a run without a K: f(is_k, seg),
// seg = the segment's lanes; f returns false to stop
template <class F>
LM_DEV void dl_segments(uint64_t mK, uint64_t mI, uint64_t mD, F&& f) {
  const uint64_t mAll = mK | mI | mD;
  uint32_t at = 0;
  while (at < 64) {
    const uint64_t rest = mAll & ~((1ull << at) - 1);
    if (!rest) break;
    const uint32_t first = (uint32_t)lmw::ffs64(rest);
    const bool is_k = (mK >> first) & 1;
    const uint64_t other = (is_k ? (mI | mD) : mK) & ~((1ull << first) - 1);
    const uint32_t end = other ? (uint32_t)lmw::ffs64(other) : 64u;
    at = end;
    if (!f(is_k, (end >= 64 ? ~0ull : (1ull << end) - 1) & ~((1ull << first) - 1))) break;
  }
}

// ---- lm_delta
LM_KERNEL void k_delta_mark(Dev d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, uint32_t* scr, DlRes* res) {
  DlRow x;
  if (!dl_mark_row(d, qs, nq, bnd, x)) return;
  if (x.ck != CK_TEXT && x.ck != CK_LIST) {
    if (dl_other_changed(x.r, x.bA, x.bV)) lmw::atomic_or(&res[x.q].other_changed, 1u);
    return;
  }
  if (x.kind == OK_DEL) dl_mark_delete(d, x, dl_bits(scr, x.Q), res);
}

LM_KERNEL LM_ONE_WAVE_GROUPS void k_delta(Dev d, const DlQuery* qs, const uint32_t* bnd, uint32_t* scr, uint8_t* out, const uint64_t* out_off, DlRes* res, int units) {
  const uint32_t q = (uint32_t)lmw::bid();
  const int lane = lmw::lane();
  const DlQuery Q = qs[q];
  const DocMeta m = d.doc[Q.doc];
  if (status_fatal(m.status)) { dl_finish(res, q, m.status, 0, 0, 0); return; }
  LM_SHARED(DlLds, s_lds, 1);
  DlLds& L = s_lds[0];
  const DlDoc D = dl_open(d, Q, m, bnd, L);
  const uint32_t* bitA = dl_bits(scr, Q);
  const uint32_t* bitV = bitA + Q.n_words;
  Sink s = dl_sink(out, out_off, q);
  int32_t err = res[q].status;   // (k_delta_mark: a delete's targets lie beyond the document's element slots)
  uint32_t n_listed = 0;
  sink_byte(s, '{');
  for (uint32_t cidx = 0; cidx < m.n_cont && !err; cidx++) {
    const ContRow o = d.cont[m.cid0 + cidx];
    const uint32_t ckind = o.kind_root & 0xff;
    if (ckind != CK_TEXT && ckind != CK_LIST) continue;
    const bool text = ckind == CK_TEXT;
    // ---- the carry: wave-uniform, across chunks and leaves
    uint32_t retain = 0, del = 0;
    bool gap = false, ins_open = false, first_item = true, cont_open = false;
    auto begin_op = [&]() {
      if (cont_open) { sink_byte(s, ','); return; }
      if (n_listed) sink_byte(s, ',');
      n_listed++;
      cont_open = true;
      if (text) sink_cid_key(s, d, m, o, ":Text\":[", 8); else sink_cid_key(s, d, m, o, ":List\":[", 8);
    };
    auto close_gap = [&]() {
      if (ins_open) { if (text) sink_lit(s, "\"}", 2); else sink_lit(s, "]}", 2); ins_open = false; }
      if (del) { begin_op(); sink_lit(s, "{\"delete\":", 10); sink_i64(s, (int64_t)del); sink_byte(s, '}'); del = 0; }
      gap = false;
    };
    dl_walk_all(d, m, cidx, D.P, L, [&](bool has, uint32_t pid, uint32_t g, uint32_t st) -> bool {
      // ---- classes
      const uint32_t pe = pid_peer(pid), ct = pid_ctr(pid);
      const bool okg = has && pe < D.P && g < Q.n_bits;
      bool in_a = false, in_vi = false;
      if (okg) {
        const uint32_t wa = bitA[g >> 5], wv = bitV[g >> 5];
        in_a = ct < L.bA[pe] && !((wa >> (g & 31)) & 1);
        in_vi = ct < L.bV[pe] && !((wv >> (g & 31)) & 1);
      }
      bool in_v = has && !(st & D.vis_mask);
      if (lmw::any((has && !okg) || (has && in_v != in_vi))) { err = ST_UNSUPPORTED; return false; }   // the self-check
      uint32_t cpv = 0;
      if (text && (in_a || in_v)) {
        bool anc;
        if (d.span) {
          const uint32_t t = d.tb[D.elem0 + g];
          anc = t == TB_ANCHOR;
          cpv = t == TB_WIDE ? d.cp[D.elem0 + g] : t;
        } else { cpv = d.cp[D.elem0 + g]; anc = cpv >= CP_ANCHOR; }
        if (anc) { in_a = false; in_v = false; cpv = 0; }
      }
      const uint64_t mK = lmw::ballot(in_a && in_v), mI = lmw::ballot(!in_a && in_v), mD = lmw::ballot(in_a && !in_v);
      const uint64_t mW = (text && units == 1) ? lmw::ballot((in_a || in_v) && cpv >= 0x10000u) : 0ull;   // one UTF-16 unit more
      dl_segments(mK, mI, mD, [&](bool is_k, uint64_t seg) -> bool {
        if (is_k) {
          if (gap) close_gap();
          retain += (uint32_t)lmw::popc64(mK & seg) + (uint32_t)lmw::popc64(mK & mW & seg);
          return true;
        }
        if (!gap) {
          if (retain) { begin_op(); sink_lit(s, "{\"retain\":", 10); sink_i64(s, (int64_t)retain); sink_byte(s, '}'); retain = 0; }
          gap = true;
        }
        del += (uint32_t)lmw::popc64(mD & seg) + (uint32_t)lmw::popc64(mD & mW & seg);
        const uint64_t im = mI & seg;
        if (!im) return true;
        if (!ins_open) {
          begin_op();
          if (text) sink_lit(s, "{\"insert\":\"", 11); else sink_lit(s, "{\"insert\":[", 11);
          ins_open = true; first_item = true;
        }
        if (text) {
          uint64_t bytes = 0;
          uint32_t nb = 0;
          if ((im >> lane) & 1) cp_bytes(cpv, bytes, nb);
          sink_lanes(s, bytes, nb);
          return true;
        }
        for (uint64_t jm = im; jm && !err; jm &= jm - 1) {
          const int l = lmw::ffs64(jm);
          const uint32_t eg = lmw::bcast(g, l), eid = lmw::bcast(pid, l);
          if (!first_item) sink_byte(s, ',');
          first_item = false;
          const uint64_t vabs = D.data0 + d.cp[D.elem0 + eg];
          if (vabs > D.end) { err = ST_INTERNAL; break; }
          Rd r = rd_make(d.data + vabs, D.end - vabs);
          uint32_t child;
          if (rd_child(r, child)) sink_child_cid(s, d, m, pid_peer(eid), pid_ctr(eid), child, err);   // a child container created by this element
          else sink_value(s, r, err, d, NONE, m.blk0, m.n_blk);
        }
        return !err;
      });
      return !err;
    });
    if (gap) close_gap();
    if (cont_open) sink_byte(s, ']');
  }
  sink_byte(s, '}');
  dl_finish(res, q, err, s.pos, n_listed, 0);
}

// the bytes of every query out of its slab (src + src_off[q], 16-byte aligned) into one dense buffer (dst + dst_off[q], 16-byte aligned;
// dst_off[q + 1] - dst_off[q] = the query's size rounded up to 16, never more than its slab): what goes back to the host is what was written
struct alignas(16) DlV16 { uint64_t a, b; };
LM_KERNEL void k_delta_pack(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off) {
  const uint32_t q = (uint32_t)lmw::bid();
  const uint64_t n = dst_off[q + 1] - dst_off[q], cap = src_off[q + 1] - src_off[q];
  const DlV16* s = (const DlV16*)(src + src_off[q]);
  DlV16* t = (DlV16*)(dst + dst_off[q]);
  for (uint64_t i = (uint64_t)lmw::lane(); i < (n < cap ? n : cap) / 16; i += 64) t[i] = s[i];
}

}  // namespace lm
