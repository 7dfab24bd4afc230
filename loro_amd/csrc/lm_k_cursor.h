// Stable cursors (include/loro_merge.h lm_cursor_pos / lm_cursor_at): LoroDoc::get_cursor_pos (loro.rs:1860-1994 → state.rs:2061-2091)
// and TextHandler / ListHandler::get_cursor (handler.rs:2673-2735, 3393-3433) answered on the device from the trackers the integrate
// stage left behind — a kernel of its own behind lm_run, like k_richtext: it reads tracker memory (leaves, directory, status words,
// cp[] / tb[]) and writes only its own result rows.
//
// Where the reference rebuilds a tracker from the oplog for a deleted element and scans it (tracker.rs:608-639, "TODO: PERF"), the
// tracker here still holds the tombstone: an id is matched against the leaf records themselves (id0 <= id < id0 + len on the items of
// its peer — no loc[], which the plain batch kernels do not keep), and the answer is the number of visible elements in front of it.
//
// One wave per document that has queries (the host lists them, Engine::cursor).  The queries of a document are grouped by
// container; the container index is looked up once per group (lane = container row).  Per group and per 64 queries — lane = query,
// the query lives in that lane's registers — ONE pass over the container's leaves in directory order, lane = item, the next leaf
// requested before this one is handled (rt_walk):
//   1  the running count of visible ELEMENTS (anchors included: the entity index) is a DPP prefix scan over the lanes' visible
//      lengths; every pending query is one readlane of its id and one ballot over the items: the hit lane's exclusive prefix, plus
//      the offset inside the run when the run is visible, is the query's entity index E.  An item that is not visible is a tombstone
//      (LM_CURSOR_DELETED) — or, under a checkout, an element the version does not hold yet (ST_FUT: LM_CURSOR_ID_NOT_FOUND);
//   2  Text only: the leaf's visible elements 64 at a time (the span-granular leaves are flattened as rt_walk flattens them), anchors
//      and scalars >= U+10000 found by ballots over tb[] / cp[]: a query whose E falls into the 64 gets pos = scalars in front of E
//      (the entity index -> event index conversion, handler.rs:2737-2745) and pos_utf16 = pos + astral scalars in front of E.
//      A List's E is its answer.
// lm_cursor_at is the same walk with step 2's test turned round: the query's position falls into the 64 -> the id of the element
// with that rank among the scalars.  Cost: one leaf pass per (container, 64 queries), never queries x document length.
#pragma once
#include "lm_k_richtext.h"

namespace lm {

// == LM_CURSOR_* in include/loro_merge.h
enum : int32_t { CUR_OK = 0, CUR_DELETED = 1, CUR_ID_NOT_FOUND = 2, CUR_CONTAINER_NOT_FOUND = 3, CUR_DOC_FAILED = 4, CUR_UNSUPPORTED = 5 };

struct CurQuery { uint64_t peer; uint32_t ctr; uint32_t has_id; };   // lm_cursor_at: ctr = the position, peer / has_id unused
struct CurGroup {            // the queries [q0, q0 + nq) of one (document, container)
  uint32_t q0, nq;
  uint32_t kind_root;        // ContRow::kind_root of the container asked for
  uint32_t counter;          // normal container: its id's counter / peer
  uint64_t peer;
  uint32_t name_off, name_len;   // root container: its name in `names`
};
struct CurRes {              // one per query, written by lane = query
  int32_t status;
  uint32_t pos, pos16;       // lm_cursor_at: the clamped position (origin_pos) in both
  uint32_t len, len16;       // the container's length at the rendered version (scalars / UTF-16 units; elements for a List)
  uint32_t ctr;              // lm_cursor_at: the element's id (has = 1)
  uint64_t peer;
  uint32_t has, pad;
};

// qdoc[b] = document of workgroup b, its groups = grp[dg0[b] .. dg0[b + 1])
LM_KERNEL void k_cursor(Dev d, const uint32_t* qdoc, const uint32_t* dg0, const CurGroup* grp, const CurQuery* qs, const uint8_t* names, CurRes* res, int at_mode) {
  const uint32_t b = (uint32_t)lmw::bid();
  const int lane = lmw::lane();
  const uint32_t doc = qdoc[b];
  const DocMeta m = d.doc[doc];
  const uint32_t g_lo = dg0[b], g_hi = dg0[b + 1];
  CurRes blank;
  blank.status = CUR_DOC_FAILED; blank.pos = 0; blank.pos16 = 0; blank.len = 0; blank.len16 = 0; blank.ctr = 0; blank.peer = 0; blank.has = 0; blank.pad = 0;
  if (status_fatal(m.status)) {
    for (uint32_t gi = g_lo; gi < g_hi; gi++) { const CurGroup G = grp[gi]; for (uint32_t q = (uint32_t)lane; q < G.nq; q += 64) res[G.q0 + q] = blank; }
    return;
  }
  const uint64_t elem0 = ((uint64_t)m.elem0_hi << 32) | m.elem0_lo;
  const bool at_version = d.res_vis && d.front_off[doc + 1] > d.front_off[doc] && !(m.flags & DF_FRONT_ERR);   // (k_richtext / k_emit_text: a resident document at a checkout)
  const uint32_t vis_mask = at_version ? (ST_FUT | ST_DELMASK) : ST_EVER;
  const bool span = d.span != 0;
  const uint32_t rec_words = span ? SP_REC : 256u, st_at = span ? 256u : 192u;
  const uint32_t P = m.n_peers < MAX_PEERS ? m.n_peers : MAX_PEERS;
  LM_SHARED(uint32_t, s_eb, MAX_PEERS);
  LM_SHARED(uint32_t, s_inc, 64);
  LM_SHARED(uint32_t, s_g0, 64);     // element slot of the item's first element, minus its exclusive prefix
  LM_SHARED(uint32_t, s_i0, 64);     // … and its id, minus the same
  for (uint32_t p = (uint32_t)lane; p < P; p += 64) s_eb[p] = d.elem_base[m.praw0 + p];
  lmw::block_sync();
  for (uint32_t gi = g_lo; gi < g_hi; gi++) {
    const CurGroup G = grp[gi];
    // ---- the container: lane = row of the document's container table
    uint32_t cidx = NONE;
    for (uint32_t c0 = 0; c0 < m.n_cont && cidx == NONE; c0 += 64) {
      const uint32_t c = c0 + (uint32_t)lane;
      bool hit = false;
      if (c < m.n_cont) {
        const ContRow o = d.cont[m.cid0 + c];
        if (o.kind_root == G.kind_root) {
          if (G.kind_root & 0x100) hit = o.name_len == G.name_len && bytes_eq(d.data + o.name_off, names + G.name_off, G.name_len);
          else hit = o.counter == G.counter && o.peer < P && d.peer_uniq[m.praw0 + o.peer] == G.peer;
        }
      }
      const uint64_t hm = lmw::ballot(hit);
      if (hm) cidx = c0 + (uint32_t)lmw::ffs64(hm);
    }
    const uint32_t kind = G.kind_root & 0xff;
    if (cidx == NONE || (kind != CK_TEXT && kind != CK_LIST)) {
      blank.status = cidx == NONE ? CUR_CONTAINER_NOT_FOUND : CUR_UNSUPPORTED;
      for (uint32_t q = (uint32_t)lane; q < G.nq; q += 64) res[G.q0 + q] = blank;
      continue;
    }
    const bool text = kind == CK_TEXT;
    const uint32_t r0 = d.cont_root0[m.cid0 + cidx], nr = d.cont_nroot[m.cid0 + cidx];
    const uint32_t* dirp = d.dir_out + m.leaf0 + r0;
    for (uint32_t qc = 0; qc < G.nq; qc += 64) {
      // ---- this lane's query.  The id's peer is looked up in the document's peer table (ascending) and packed like the items' ids
      const bool mine = qc + (uint32_t)lane < G.nq;
      CurQuery Q;
      Q.peer = 0; Q.ctr = 0; Q.has_id = 0;
      if (mine) Q = qs[G.q0 + qc + (uint32_t)lane];
      uint32_t my_pid = NONE;
      if (!at_mode && mine && Q.has_id && Q.ctr < MAX_COUNTER) {
        uint32_t lo = 0, hi = P;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (d.peer_uniq[m.praw0 + mid] < Q.peer) lo = mid + 1; else hi = mid; }
        if (lo < P && d.peer_uniq[m.praw0 + lo] == Q.peer) my_pid = pid_make(lo, Q.ctr);
      }
      int32_t my_st = CUR_ID_NOT_FOUND;
      uint32_t my_E = 0, my_pos = 0, my_p16 = 0, my_id = NONE;
      bool my_conv = false;                                   // E is known, pos / pos16 are not yet (Text)
      bool my_wait = at_mode ? mine : false;                  // lm_cursor_at: no element found yet
      uint64_t pend = lmw::ballot(my_pid != NONE);            // lm_cursor_pos: queries not matched against an item yet
      uint32_t vis_before = 0, n_sc = 0, n_as = 0;            // visible elements / scalars / astral scalars in front of this leaf (batch)
      // ---- the walk (rt_walk's prefetch: the record of the next leaf and the directory entry behind it are on their way)
      uint32_t de1 = nr > 0 ? dirp[0] : 0u, de2 = nr > 1 ? dirp[1] : 0u;
      uint32_t p_id = NONE, p_ln = 1, p_st = ST_EVER;
      if (nr > 0 && (uint32_t)lane < de_n(de1)) {
        const uint32_t* rec = d.it + (uint64_t)(m.leaf0 + de_leaf(de1)) * rec_words;
        p_id = rec[lane]; p_st = rec[st_at + lane]; if (span) p_ln = rec[64 + lane];
      }
      for (uint32_t ri = 0; ri < nr; ri++) {
        const uint32_t id0 = p_id, ln = p_ln, st = p_st;
        de1 = de2;
        de2 = ri + 2 < nr ? dirp[ri + 2] : 0u;
        p_id = NONE; p_ln = 1; p_st = ST_EVER;
        if (ri + 1 < nr && (uint32_t)lane < de_n(de1)) {
          const uint32_t* rec = d.it + (uint64_t)(m.leaf0 + de_leaf(de1)) * rec_words;
          p_id = rec[lane]; p_st = rec[st_at + lane]; if (span) p_ln = rec[64 + lane];
        }
        const bool in = id0 != NONE;
        const bool vis = in && !(st & vis_mask);
        const uint32_t vl = vis ? ln : 0u;
        const uint32_t inc = lmw::scan_incl_add(vl);
        const uint32_t excl = inc - vl;
        const uint32_t total = lmw::bcast(inc, 63);
        // ---- 1: ids against items
        const uint64_t vism = lmw::ballot(vis);
        for (uint64_t pm = pend; pm; pm &= pm - 1) {
          const int q = lmw::ffs64(pm);
          const uint32_t qpid = lmw::bcast(my_pid, q);
          const uint64_t hm = lmw::ballot(in && qpid - id0 < ln);   // (same peer: an item never crosses its peer's 2^24 counters)
          if (!hm) continue;
          const int h = lmw::ffs64(hm);
          const bool hv = (vism >> h) & 1;
          const uint32_t hst = lmw::bcast(st, h);
          const uint32_t E = vis_before + lmw::bcast(excl, h) + (hv ? qpid - lmw::bcast(id0, h) : 0u);
          const bool gone = !hv && at_version && (hst & ST_FUT);    // the version does not hold the element (yet)
          if (lane == q) { my_E = E; my_st = hv ? CUR_OK : gone ? CUR_ID_NOT_FOUND : CUR_DELETED; my_conv = !gone; }
          pend &= ~(1ull << q);
        }
        // ---- 2: the leaf's visible elements, 64 at a time
        if ((text || at_mode) && total) {
          if (span) {
            lmw::block_sync();
            s_inc[lane] = inc;
            s_g0[lane] = vl ? s_eb[pid_peer(id0)] + pid_ctr(id0) - excl : 0u;
            s_i0[lane] = vl ? id0 - excl : 0u;
            lmw::block_sync();
          }
          for (uint32_t e0 = 0; e0 < (span ? total : 1u); e0 += 64) {
            bool has;
            uint32_t rank, g = 0, pid = NONE;   // rank: index among the leaf's visible elements
            if (span) {
              rank = e0 + (uint32_t)lane;
              has = rank < total;
              if (has) {
                uint32_t lo = 0, hi = 63;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_inc[mid] > rank) hi = mid; else lo = mid + 1; }
                g = s_g0[lo] + rank; pid = s_i0[lo] + rank;
              }
            } else {
              has = vis; rank = excl; pid = id0;
              if (has) g = s_eb[pid_peer(id0)] + pid_ctr(id0);
            }
            bool anc = false, astral = false;
            if (has && text) {
              if (span) {
                const uint32_t t = d.tb[elem0 + g];
                anc = t == TB_ANCHOR;
                astral = t == TB_WIDE && d.cp[elem0 + g] >= 0x10000u;
              } else {
                const uint32_t cpv = d.cp[elem0 + g];
                anc = cpv >= CP_ANCHOR;
                astral = !anc && cpv >= 0x10000u;
              }
            }
            const uint32_t arank = vis_before + rank;                         // the element's entity index
            const uint32_t b_hi = vis_before + (span ? (e0 + 64 < total ? e0 + 64 : total) : total);
            const uint64_t scm = lmw::ballot(has && !anc), asm_ = lmw::ballot(has && astral);
            if (!at_mode) {
              for (uint64_t cm = lmw::ballot(my_conv && my_E < b_hi); cm; cm &= cm - 1) {
                const int q = lmw::ffs64(cm);
                const uint32_t E = lmw::bcast(my_E, q);
                const uint32_t sc = n_sc + (uint32_t)lmw::popc64(lmw::ballot(has && !anc && arank < E));
                const uint32_t as = n_as + (uint32_t)lmw::popc64(lmw::ballot(has && astral && arank < E));
                if (lane == q) { my_pos = sc; my_p16 = sc + as; my_conv = false; }
              }
            } else {
              const uint32_t srank = n_sc + (uint32_t)lmw::popc64(scm & ((1ull << lane) - 1));   // the scalar's index (lanes are in sequence order)
              const uint32_t sc_hi = n_sc + (uint32_t)lmw::popc64(scm);
              for (uint64_t cm = lmw::ballot(my_wait && Q.ctr < sc_hi); cm; cm &= cm - 1) {
                const int q = lmw::ffs64(cm);
                const uint32_t want = lmw::bcast(Q.ctr, q);
                const uint64_t hm = lmw::ballot(has && !anc && srank == want);
                const int h = hm ? lmw::ffs64(hm) : 0;
                const uint32_t idv = lmw::bcast(pid, h);
                if (lane == q) { my_id = hm ? idv : NONE; my_wait = false; }
              }
            }
            n_sc += (uint32_t)lmw::popc64(scm);
            n_as += (uint32_t)lmw::popc64(asm_);
          }
        }
        vis_before += total;
      }
      // ---- the rows
      if (!text && !at_mode) n_sc = vis_before;
      if (mine) {
        CurRes R;
        R.len = n_sc; R.len16 = n_sc + n_as; R.has = 0; R.pad = 0; R.ctr = 0; R.peer = 0;
        if (at_mode) {
          const bool found = my_id != NONE && pid_peer(my_id) < P;
          R.status = CUR_OK;
          R.pos = R.pos16 = found ? Q.ctr : n_sc;
          if (found) { R.has = 1; R.ctr = pid_ctr(my_id); R.peer = d.peer_uniq[m.praw0 + pid_peer(my_id)]; }
        } else if (!Q.has_id) {
          R.status = CUR_OK; R.pos = n_sc; R.pos16 = n_sc + n_as;     // (the host turns Left into 0, state.rs:2073-2090)
        } else {
          if (my_conv) { my_pos = n_sc; my_p16 = n_sc + n_as; }       // E = every visible element: behind the last scalar
          if (!text) { my_pos = my_E; my_p16 = my_E; }
          const bool ans = my_st == CUR_OK || my_st == CUR_DELETED;
          R.status = my_st; R.pos = ans ? my_pos : 0u; R.pos16 = ans ? my_p16 : 0u;
        }
        res[G.q0 + qc + (uint32_t)lane] = R;
      }
    }
  }
}

}  // namespace lm
