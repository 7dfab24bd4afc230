// Text / List deltas between two versions (include/loro_merge.h lm_delta): what LoroDoc::diff(a, b) and the TextDelta / ListDiffItem
// events of subscribe tell a subscriber, answered on the device from the trackers and op rows the last run left — kernels of their
// own behind lm_run, like k_richtext and k_cursor: they read tracker memory (leaves, directory, status words, cp[] / tb[]) and the
// decoded op rows, and write only their own bitmaps, slabs and result rows.
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
//               query indexed by element slot (elem_base[peer] + counter): deleted-in-A and deleted-in-V, word-wise atomic_or, one
//               mask per touched word.  Rows of containers of other kinds whose id lies in V \ A raise the query's other_changed.
// k_delta       one wave per query; per Text / List container the leaves in directory order (k_cursor's walk for both layouts, the
//               next leaf requested before this one is handled), 64 elements per step, classes by ballots.  SELF-CHECK: "in V by
//               status" must equal "c < V[p] and bit V clear" for every element — a mismatch (a delete applied by position, a damaged
//               document, anything not thought of) gives the query LM_UNSUPPORTED: the right value or a refusal, never a guess.
//               Class runs are coalesced across chunk and leaf boundaries through a wave-uniform carry (the retain count, whether a
//               gap / an insert is open, the pending delete count).  Text inserts are escaped and stored by all lanes at once
//               (cp_bytes + sink_lanes: the emitter's escapes, lengths by a DPP prefix scan), List values go through the emitter's
//               value sink one after the other.  Output goes into optimistic per-query slabs; the kernel never writes beyond a slab
//               and always reports the exact size (Engine::delta launches a second time at exact sizes when one overflowed).
// k_delta_pack  one wave per query: the written bytes out of the slabs into one dense buffer — only that buffer goes to the host.
#pragma once
#include "lm_k_cursor.h"

namespace lm {

struct DlQuery {
  uint32_t doc;
  uint32_t n_bnd;       // peers of the document: A[p] = bnd[bnd0 + p], V[p] = bnd[bnd0 + n_bnd + p] (decoded by the host)
  uint64_t bnd0;
  uint64_t bits0;       // word index of the deleted-in-A bitmap; deleted-in-V follows n_words behind it
  uint32_t n_words;
  uint32_t n_bits;      // element slots the bitmaps cover
  uint32_t row_blk0;    // k_delta_mark: first workgroup of this query (ascending over the queries)
  uint32_t pad;
};
struct DlRes {          // one per query; cleared by the host in front of k_delta_mark
  int32_t status;
  uint32_t other_changed;
  uint32_t len;         // exact size of the query's JSON
  uint32_t cnt;         // members written (the host orders them)
};

LM_KERNEL void k_delta_mark(Dev d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, uint32_t* bits, DlRes* res) {
  const uint32_t b = (uint32_t)lmw::bid();
  uint32_t lo = 0, hi = nq;   // the last query whose first workgroup is at or in front of this one (a query without rows owns none)
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (qs[mid].row_blk0 <= b) lo = mid; else hi = mid; }
  const DlQuery Q = qs[lo];
  const DocMeta m = d.doc[Q.doc];
  const uint32_t i = (b - Q.row_blk0) * 64 + (uint32_t)lmw::lane();
  if (i >= m.n_op) return;
  const OpRow r = d.op[m.op0 + i];
  const uint32_t kind = (r.cidx_kind >> 16) & 0xff, cidx = r.cidx_kind & 0xffff;
  const uint32_t peer = d.chg[r.chg].peer;
  if (cidx >= m.n_cont || peer >= Q.n_bnd) return;
  const uint32_t bA = bnd[Q.bnd0 + peer], bV = bnd[Q.bnd0 + Q.n_bnd + peer];
  const uint32_t ck = d.cont[m.cid0 + cidx].kind_root & 0xff;
  if (ck != CK_TEXT && ck != CK_LIST) {
    if (r.ctr < bV && (uint64_t)r.ctr + (r.len ? r.len : 1u) > bA) lmw::atomic_or(&res[lo].other_changed, 1u);
    return;
  }
  if (kind != OK_DEL || r.a0 >= Q.n_bnd) return;
  const uint32_t Ln = (uint32_t)(r.a2 < 0 ? -r.a2 : r.a2);
  const uint32_t eb = d.elem_base[m.praw0 + r.a0];
  for (int pass = 0; pass < 2; pass++) {
    const uint32_t bound = pass ? bV : bA;
    if (bound <= r.ctr) continue;
    uint32_t nb = bound - r.ctr;                      // the row's atoms [0, nb) have ids below the bound
    if (nb > r.len) nb = r.len;
    if (nb > Ln) nb = Ln;
    if (!nb) continue;
    const uint64_t g0 = (uint64_t)eb + r.a1 + (r.a2 > 0 ? 0u : Ln - nb), g1 = g0 + nb;   // (lm_k_integrate_span.h: a backspace run targets its range back to front)
    if (g1 > Q.n_bits) { (void)lmw::atomic_max32((uint32_t*)&res[lo].status, (uint32_t)ST_UNSUPPORTED); continue; }
    uint32_t* w = bits + Q.bits0 + (pass ? Q.n_words : 0u);
    const uint32_t w0 = (uint32_t)(g0 >> 5), w1 = (uint32_t)((g1 - 1) >> 5);
    for (uint32_t k = w0; k <= w1; k++) {
      const uint32_t lo_b = k == w0 ? (uint32_t)(g0 & 31) : 0u, hi_b = k == w1 ? (uint32_t)((g1 - 1) & 31) + 1u : 32u;
      const uint32_t mask = (hi_b == 32 ? 0xFFFFFFFFu : (1u << hi_b) - 1u) & ~((1u << lo_b) - 1u);
      (void)lmw::atomic_or(w + k, mask);
    }
  }
}

LM_KERNEL LM_ONE_WAVE_GROUPS void k_delta(Dev d, const DlQuery* qs, const uint32_t* bnd, const uint32_t* bits, uint8_t* out, const uint64_t* out_off, DlRes* res, int units) {
  const uint32_t q = (uint32_t)lmw::bid();
  const int lane = lmw::lane();
  const DlQuery Q = qs[q];
  const uint32_t doc = Q.doc;
  const DocMeta m = d.doc[doc];
  if (status_fatal(m.status)) { if (lane == 0) { res[q].status = m.status; res[q].len = 0; res[q].cnt = 0; } return; }
  const uint64_t elem0 = ((uint64_t)m.elem0_hi << 32) | m.elem0_lo;
  const bool at_version = d.res_vis && d.front_off[doc + 1] > d.front_off[doc] && !(m.flags & DF_FRONT_ERR);   // (k_cursor / k_emit_text)
  const uint32_t vis_mask = at_version ? (ST_FUT | ST_DELMASK) : ST_EVER;
  const bool span = d.span != 0;
  const uint32_t rec_words = span ? SP_REC : 256u, st_at = span ? 256u : 192u;
  const uint32_t P = m.n_peers < Q.n_bnd ? m.n_peers : Q.n_bnd;
  const uint32_t* bitA = bits + Q.bits0;
  const uint32_t* bitV = bitA + Q.n_words;
  const uint64_t doc_data0 = d.blob_off[d.doc_blob[doc]];
  uint64_t doc_end = 0;   // list item values are bounded by the end of the document's last blob (k_emit_any)
  if (d.doc_blob[doc + 1] > d.doc_blob[doc]) doc_end = d.blob_off[d.doc_blob[doc + 1] - 1] + d.blob_len[d.doc_blob[doc + 1] - 1];
  LM_SHARED(uint32_t, s_eb, MAX_PEERS);
  LM_SHARED(uint32_t, s_bA, MAX_PEERS);
  LM_SHARED(uint32_t, s_bV, MAX_PEERS);
  LM_SHARED(uint32_t, s_inc, 64);
  LM_SHARED(uint32_t, s_g0, 64);     // element slot of the item's first element, minus its exclusive prefix
  LM_SHARED(uint32_t, s_i0, 64);     // … its id, minus the same
  LM_SHARED(uint32_t, s_st, 64);     // … and its status word
  for (uint32_t p = (uint32_t)lane; p < MAX_PEERS; p += 64) {
    s_eb[p] = p < P ? d.elem_base[m.praw0 + p] : 0u;
    s_bA[p] = p < P ? bnd[Q.bnd0 + p] : 0u;
    s_bV[p] = p < P ? bnd[Q.bnd0 + Q.n_bnd + p] : 0u;
  }
  lmw::block_sync();
  Sink s;
  s.out = out + out_off[q];
  s.pos = 0;
  s.cap = out_off[q + 1] - out_off[q];
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
      if (o.kind_root & 0x100) {
        sink_lit(s, "\"cid:root-", 10);
        sink_escaped(s, d.data + o.name_off, o.name_len);
      } else {
        sink_lit(s, "\"cid:", 5);
        sink_i64(s, (int64_t)(int32_t)o.counter);
        sink_byte(s, '@');
        sink_u64(s, o.peer < m.n_peers ? d.peer_uniq[m.praw0 + o.peer] : 0ull);
      }
      if (text) sink_lit(s, ":Text\":[", 8); else sink_lit(s, ":List\":[", 8);
    };
    auto close_gap = [&]() {
      if (ins_open) { if (text) sink_lit(s, "\"}", 2); else sink_lit(s, "]}", 2); ins_open = false; }
      if (del) { begin_op(); sink_lit(s, "{\"delete\":", 10); sink_i64(s, (int64_t)del); sink_byte(s, '}'); del = 0; }
      gap = false;
    };
    // ---- the walk (k_cursor's: the record of the next leaf and the directory entry behind it are on their way)
    const uint32_t r0 = d.cont_root0[m.cid0 + cidx], nr = d.cont_nroot[m.cid0 + cidx];
    const uint32_t* dirp = d.dir_out + m.leaf0 + r0;
    uint32_t de1 = nr > 0 ? dirp[0] : 0u, de2 = nr > 1 ? dirp[1] : 0u;
    uint32_t p_id = NONE, p_ln = 1, p_st = ST_EVER;
    if (nr > 0 && (uint32_t)lane < de_n(de1)) {
      const uint32_t* rec = d.it + (uint64_t)(m.leaf0 + de_leaf(de1)) * rec_words;
      p_id = rec[lane]; p_st = rec[st_at + lane]; if (span) p_ln = rec[64 + lane];
    }
    for (uint32_t ri = 0; ri < nr && !err; ri++) {
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
      if (span) {   // every element of the leaf, tombstones included, 64 at a time
        const uint32_t al = in ? ln : 0u;
        const uint32_t inc = lmw::scan_incl_add(al);
        total = lmw::bcast(inc, 63);
        lmw::block_sync();
        s_inc[lane] = inc;
        s_g0[lane] = al && pid_peer(id0) < P ? s_eb[pid_peer(id0)] + pid_ctr(id0) - (inc - al) : 0u;
        s_i0[lane] = al ? id0 - (inc - al) : 0u;
        s_st[lane] = st0;
        lmw::block_sync();
      } else if (!lmw::any(in)) continue;
      for (uint32_t e0 = 0; e0 < total && !err; e0 += 64) {
        bool has;
        uint32_t pid = NONE, g = 0, st = ST_EVER;
        if (span) {
          const uint32_t e = e0 + (uint32_t)lane;
          has = e < total;
          if (has) {
            uint32_t lo = 0, hi = 63;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_inc[mid] > e) hi = mid; else lo = mid + 1; }
            g = s_g0[lo] + e; pid = s_i0[lo] + e; st = s_st[lo];
          }
        } else {
          has = in; pid = id0; st = st0;
          if (has && pid_peer(id0) < P) g = s_eb[pid_peer(id0)] + pid_ctr(id0);
        }
        // ---- classes
        const uint32_t pe = pid_peer(pid), ct = pid_ctr(pid);
        const bool okg = has && pe < P && g < Q.n_bits;
        bool in_a = false, in_vi = false;
        if (okg) {
          const uint32_t wa = bitA[g >> 5], wv = bitV[g >> 5];
          in_a = ct < s_bA[pe] && !((wa >> (g & 31)) & 1);
          in_vi = ct < s_bV[pe] && !((wv >> (g & 31)) & 1);
        }
        bool in_v = has && !(st & vis_mask);
        if (lmw::any((has && !okg) || (has && in_v != in_vi))) { err = ST_UNSUPPORTED; break; }   // the self-check
        uint32_t cpv = 0;
        if (text && (in_a || in_v)) {
          bool anc;
          if (span) {
            const uint32_t t = d.tb[elem0 + g];
            anc = t == TB_ANCHOR;
            cpv = t == TB_WIDE ? d.cp[elem0 + g] : t;
          } else { cpv = d.cp[elem0 + g]; anc = cpv >= CP_ANCHOR; }
          if (anc) { in_a = false; in_v = false; cpv = 0; }
        }
        const uint64_t mK = lmw::ballot(in_a && in_v), mI = lmw::ballot(!in_a && in_v), mD = lmw::ballot(in_a && !in_v);
        const uint64_t mW = (text && units == 1) ? lmw::ballot((in_a || in_v) && cpv >= 0x10000u) : 0ull;   // one UTF-16 unit more
        const uint64_t mAll = mK | mI | mD;
        uint32_t at = 0;
        while (at < 64 && !err) {
          const uint64_t rest = mAll & ~((1ull << at) - 1);
          if (!rest) break;
          const uint32_t f = (uint32_t)lmw::ffs64(rest);
          const bool is_k = (mK >> f) & 1;
          const uint64_t other = (is_k ? (mI | mD) : mK) & ~((1ull << f) - 1);
          const uint32_t end = other ? (uint32_t)lmw::ffs64(other) : 64u;
          const uint64_t seg = (end >= 64 ? ~0ull : (1ull << end) - 1) & ~((1ull << f) - 1);
          at = end;
          if (is_k) {
            if (gap) close_gap();
            retain += (uint32_t)lmw::popc64(mK & seg) + (uint32_t)lmw::popc64(mK & mW & seg);
            continue;
          }
          if (!gap) {
            if (retain) { begin_op(); sink_lit(s, "{\"retain\":", 10); sink_i64(s, (int64_t)retain); sink_byte(s, '}'); retain = 0; }
            gap = true;
          }
          del += (uint32_t)lmw::popc64(mD & seg) + (uint32_t)lmw::popc64(mD & mW & seg);
          const uint64_t im = mI & seg;
          if (!im) continue;
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
            continue;
          }
          for (uint64_t jm = im; jm && !err; jm &= jm - 1) {
            const int l = lmw::ffs64(jm);
            const uint32_t eg = lmw::bcast(g, l), eid = lmw::bcast(pid, l);
            if (!first_item) sink_byte(s, ',');
            first_item = false;
            const uint64_t vabs = doc_data0 + d.cp[elem0 + eg];
            if (vabs > doc_end) { err = ST_INTERNAL; break; }
            Rd r = rd_make(d.data + vabs, doc_end - vabs);
            if (r.p < r.end && *r.p == 9) {   // a child container created by this element: LoroValue::Container, never its content
              (void)rd_u8(r);
              const uint32_t child = rd_u8(r);
              sink_lit(s, "\"\xF0\x9F\xA6\x9C:cid:", 10);
              sink_i64(s, (int64_t)pid_ctr(eid));
              sink_byte(s, '@');
              sink_u64(s, d.peer_uniq[m.praw0 + pid_peer(eid)]);
              if (child == CK_MAP) sink_lit(s, ":Map\"", 5);
              else if (child == CK_LIST) sink_lit(s, ":List\"", 6);
              else if (child == CK_TEXT) sink_lit(s, ":Text\"", 6);
              else if (child == CK_TREE) sink_lit(s, ":Tree\"", 6);
              else if (child == CK_MOVABLE) sink_lit(s, ":MovableList\"", 13);
              else if (child == CK_COUNTER) sink_lit(s, ":Counter\"", 9);
              else err = ST_UNSUPPORTED;
              continue;
            }
            sink_value(s, r, err, d, NONE, m.blk0, m.n_blk);
          }
        }
      }
    }
    if (gap) close_gap();
    if (cont_open) sink_byte(s, ']');
  }
  sink_byte(s, '}');
  if (lane == 0) {
    res[q].status = err ? err : (int32_t)ST_OK;
    res[q].len = err ? 0u : (uint32_t)s.pos;   // (s.pos > s.cap: the host sees the size and launches again with room for it)
    res[q].cnt = n_listed;
  }
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
