// MovableList deltas between two versions (include/loro_merge.h lm_delta_movable): what LoroDoc::diff(a, b) and the ListDiffItem events
// of subscribe tell a subscriber about the MovableList containers — retain / insert (with from_move) / delete — answered on the device
// from what the last run left: the trackers (every ITEM of a MovableList, placed by an insert or by a move, tombstones included, in a
// sequence order that does not depend on the version), loc[item] = the element the item positions (k_mlist_post), the per-element
// maxima of the moves and sets at V in the document's table (ht_key / ht_best, ml_key) and the op rows.  Kernels of their own behind
// lm_run, like k_delta and k_mdelta: they write only their own bitmaps, winner words, slabs and result rows.
//
// A = the version the subscriber has (the query's from_vv), V = the version the run rendered; both are ID SETS, A inside V.
//   pos_X(e) = the greatest, by (lamport, peer), of e's insert and its moves whose ids lie in X;  val_X(e) likewise over its sets
//   item i SHOWS at X  iff  id(i) in X, i is pos_X(el(i)), and no delete atom whose own id lies in X targets i
// (a move deletes the item it took the element from; the winner of X is never such an item, so "deleted" below may and does include
// "taken by a move in X" — that makes the bitmap at V equal to the tracker's status words, which is the self-check).
//   K  shows at A and at V, value unchanged          R  shows at both, value changed: one delete and one insert in place
//   I  shows at V only                               D  shows at A only
//   an I carries from_move iff its element shows at A (at another item, which is then a D) and its value is unchanged
// "value unchanged": val_A(e) and val_V(e) are the same op, or their values are equal under LoroValue equality (md_value_eq); a pair that
// function does not decide (two nested List / Map values) counts as changed and sets bit 1 of other_changed.  Canonical form: lm_delta's
// (a maximal K run -> retain; in a gap all inserts in sequence order, consecutive ones with the same flag in one op, then one delete).
//
// k_mldelta_mark lane = op row, k_delta_mark's grid.  Rows of MovableList containers: a delete row sets its targets' bits in the
//                deleted-in-A / deleted-in-V bitmaps (word-wise masks, a version may cut the row, a backspace run goes back to front);
//                a move row sets the bit of the item it took the element from (the integrate kernels left its id in the move item's
//                cp[] slot) and raises the element's move winner; a set row raises its set winner.  Winner words are indexed by the
//                slot the element's key (ml_key) has in the document's table and raised by atomic_max64 of k_mlist_post's packed word
//                (lamport, peer index, row) + 1 — winV for rows below V, winA for rows below A.  Duplicate blobs are idempotent: the
//                same (lamport, peer) from another row.  Rows of Tree / Counter containers with an id in V \ A set bit 0.
// k_mldelta      one wave per query; per MovableList container k_delta's leaf walk (both tracker layouts, the next leaf requested in
//                front, span leaves flattened 64 items at a time).  SELF-CHECK, the right value or a refusal (LM_UNSUPPORTED):
//                (a) for every item "visible by status word" == "id below V and bit V clear";
//                (b) for every element of an item in V the move and set winners at V raised from the op rows name the ops the run
//                    left in the document's table (compared without the row index: a duplicated blob holds the op in two rows).
//                Classes by ballots, k_delta's wave-uniform carry, values through the emitter's sink.  Output goes into optimistic
//                per-query slabs; the kernel never writes beyond a slab and always reports the exact size.
// k_delta_pack   (lm_k_delta.h) moves the written bytes into one dense buffer.
//
// The query's words (DlQuery, as Engine::delta_movable fills it): bits0 = first 64-bit word of the query's scratch, pad = the slots of
// the document's table (cap), n_words = 32-bit words of one bitmap, n_bits = the element slots it covers.  Scratch: winV[cap], winA[cap],
// then deleted-in-A[n_words], deleted-in-V[n_words].
#pragma once
#include "lm_k_delta_map.h"

namespace lm {

// two packed winner words name the same op (or both name none): the row index in the low 24 bits is left out
LM_DEV bool mld_same(unsigned long long a, unsigned long long b) {
  if (a == 0 || b == 0) return a == b;
  return ((a - 1) >> 24) == ((b - 1) >> 24);
}

LM_KERNEL void k_mldelta_mark(Dev d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, unsigned long long* win, DlRes* res) {
  const uint32_t b = (uint32_t)lmw::bid();
  uint32_t lo = 0, hi = nq;   // (k_delta_mark: the last query whose first workgroup is at or in front of this one)
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (qs[mid].row_blk0 <= b) lo = mid; else hi = mid; }
  const DlQuery Q = qs[lo];
  const DocMeta m = d.doc[Q.doc];
  const uint32_t i = (b - Q.row_blk0) * 64 + (uint32_t)lmw::lane();
  if (i >= m.n_op || status_fatal(m.status)) return;
  const OpRow r = d.op[m.op0 + i];
  const uint32_t kind = (r.cidx_kind >> 16) & 0xff, cidx = r.cidx_kind & 0xffff;
  const ChangeRow ch = d.chg[r.chg];
  const uint32_t peer = ch.peer;
  if (cidx >= m.n_cont || peer >= Q.n_bnd) return;
  const uint32_t bA = bnd[Q.bnd0 + peer], bV = bnd[Q.bnd0 + Q.n_bnd + peer];
  const uint32_t ck = d.cont[m.cid0 + cidx].kind_root & 0xff;
  if (ck == CK_TREE || ck == CK_COUNTER) {
    if (r.ctr < bV && (uint64_t)r.ctr + (r.len ? r.len : 1u) > bA) lmw::atomic_or(&res[lo].other_changed, 1u);
    return;
  }
  if (ck != CK_MOVABLE) return;
  const uint32_t cap = Q.pad;
  unsigned long long* winV = win + Q.bits0;
  uint32_t* bits = (uint32_t*)(winV + 2ull * cap);
  auto refuse = [&]() { (void)lmw::atomic_max32((uint32_t*)&res[lo].status, (uint32_t)ST_UNSUPPORTED); };
  // items [g0, g1) are gone at the versions whose bound reaches beyond the row's atom `need - 1`
  auto mark = [&](int pass, uint64_t g0, uint64_t g1) {
    if (g1 > Q.n_bits) { refuse(); return; }
    uint32_t* w = bits + (pass ? Q.n_words : 0u);
    const uint32_t w0 = (uint32_t)(g0 >> 5), w1 = (uint32_t)((g1 - 1) >> 5);
    for (uint32_t k = w0; k <= w1; k++) {
      const uint32_t lo_b = k == w0 ? (uint32_t)(g0 & 31) : 0u, hi_b = k == w1 ? (uint32_t)((g1 - 1) & 31) + 1u : 32u;
      const uint32_t mask = (hi_b == 32 ? 0xFFFFFFFFu : (1u << hi_b) - 1u) & ~((1u << lo_b) - 1u);
      (void)lmw::atomic_or(w + k, mask);
    }
  };
  if (kind == OK_DEL) {
    if (r.a0 >= Q.n_bnd) return;
    const uint32_t Ln = (uint32_t)(r.a2 < 0 ? -r.a2 : r.a2);
    const uint32_t eb = d.elem_base[m.praw0 + r.a0];
    for (int pass = 0; pass < 2; pass++) {
      const uint32_t bound = pass ? bV : bA;
      if (bound <= r.ctr) continue;
      uint32_t nb = bound - r.ctr;                      // the row's atoms [0, nb) have ids below the bound
      if (nb > r.len) nb = r.len;
      if (nb > Ln) nb = Ln;
      if (!nb) continue;
      const uint64_t g0 = (uint64_t)eb + r.a1 + (r.a2 > 0 ? 0u : Ln - nb);   // (k_delta_mark: a backspace run targets its range back to front)
      mark(pass, g0, g0 + nb);
    }
    return;
  }
  if (kind != OK_LIST_MOVE && kind != OK_LIST_SET) return;
  if (r.ctr >= bV) return;                              // beyond the rendered version: does not compete
  if (cap == 0 || cap != d.ht_cap[Q.doc] || i >= (1u << 24) || peer >= 256u) { refuse(); return; }
  const uint32_t pid_e = ml_resolve(d, m, cidx, r.a0, r.a1);
  if (pid_e == NONE) { refuse(); return; }
  if (kind == OK_LIST_MOVE) {                           // the item the move took the element from (lm_k_integrate*.h: the move item's cp[] slot)
    const uint64_t gm = (uint64_t)d.elem_base[m.praw0 + peer] + r.ctr;
    if (gm >= Q.n_bits || gm >= m.atoms) { refuse(); return; }
    const uint32_t tgt = (d.cp + (((uint64_t)m.elem0_hi << 32) | m.elem0_lo))[gm];
    if (tgt == NONE || pid_peer(tgt) >= Q.n_bnd) { refuse(); return; }
    const uint64_t gt = (uint64_t)d.elem_base[m.praw0 + pid_peer(tgt)] + pid_ctr(tgt);
    mark(1, gt, gt + 1);
    if (r.ctr < bA) mark(0, gt, gt + 1);
  }
  const uint32_t slot = ml_ht_find(d.ht_key + d.ht0[Q.doc], cap, ml_key(pid_e, kind == OK_LIST_SET));
  if (slot == NONE) { refuse(); return; }
  const unsigned long long v = (((unsigned long long)(d.chg_lamport[r.chg] + (r.ctr - ch.ctr)) << 32) | ((unsigned long long)peer << 24) | i) + 1;
  unsigned long long* wV = winV + slot;
  if (*wV < v) (void)lmw::atomic_max64(wV, v);
  if (r.ctr < bA && wV[cap] < v) (void)lmw::atomic_max64(wV + cap, v);
}

LM_KERNEL LM_ONE_WAVE_GROUPS void k_mldelta(Dev d, const DlQuery* qs, const uint32_t* bnd, const unsigned long long* win, uint8_t* out, const uint64_t* out_off, DlRes* res) {
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
  const uint32_t cap = Q.pad;
  const unsigned long long* winV = win + Q.bits0;
  const unsigned long long* winA = winV + cap;
  const uint32_t* bitA = (const uint32_t*)(winV + 2ull * cap);
  const uint32_t* bitV = bitA + Q.n_words;
  const unsigned long long* keys = d.ht_key + d.ht0[doc];
  const unsigned long long* best = d.ht_best + d.ht0[doc];
  const uint32_t* loc = d.loc + elem0;
  const uint64_t doc_data0 = d.blob_off[d.doc_blob[doc]];
  uint64_t doc_end = 0;   // inserted values are bounded by the end of the document's last blob (k_emit_any)
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
  int32_t err = res[q].status;   // (k_mldelta_mark: a target beyond the element slots, a key the table does not hold)
  if (!err && cap != d.ht_cap[doc]) err = ST_UNSUPPORTED;
  uint32_t n_listed = 0, undecided = 0;
  // slot of an item id, NONE when it lies beyond the bitmaps
  auto slot_of = [&](uint32_t id) -> uint32_t {
    if (id == NONE || pid_peer(id) >= P) return NONE;
    const uint64_t g = (uint64_t)s_eb[pid_peer(id)] + pid_ctr(id);
    return g < Q.n_bits && g < m.atoms ? (uint32_t)g : NONE;
  };
  // the item a packed move winner placed
  auto item_of = [&](unsigned long long w) -> uint32_t {
    const uint32_t row = (uint32_t)((w - 1) & 0xffffffu);
    return row < m.n_op ? pid_make((uint32_t)((w - 1) >> 24) & 0xffu, d.op[m.op0 + row].ctr) : NONE;
  };
  sink_byte(s, '{');
  for (uint32_t cidx = 0; cidx < m.n_cont && !err; cidx++) {
    const ContRow o = d.cont[m.cid0 + cidx];
    if ((o.kind_root & 0xff) != CK_MOVABLE) continue;
    // ---- the carry: wave-uniform, across chunks and leaves
    uint32_t retain = 0, del = 0;
    bool gap = false, ins_open = false, ins_flag = false, first_item = true, cont_open = false;
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
      sink_lit(s, ":MovableList\":[", 15);
    };
    auto close_ins = [&]() {
      if (!ins_open) return;
      if (ins_flag) sink_lit(s, "],\"from_move\":true}", 19); else sink_lit(s, "]}", 2);
      ins_open = false;
    };
    auto close_gap = [&]() {
      close_ins();
      if (del) { begin_op(); sink_lit(s, "{\"delete\":", 10); sink_i64(s, (int64_t)del); sink_byte(s, '}'); del = 0; }
      gap = false;
    };
    // ---- the walk (k_delta's: the record of the next leaf and the directory entry behind it are on their way)
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
      if (span) {   // every item of the leaf, tombstones included, 64 at a time
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
        // ---- the item: in A / in V by id, gone at A / at V by the bitmaps
        const uint32_t pe = pid_peer(pid), ct = pid_ctr(pid);
        const bool okg = has && pe < P && g < Q.n_bits && g < m.atoms;
        bool id_a = false, id_v = false, gone_a = false, gone_v = false;
        if (okg) {
          id_a = ct < s_bA[pe]; id_v = ct < s_bV[pe];
          gone_a = (bitA[g >> 5] >> (g & 31)) & 1; gone_v = (bitV[g >> 5] >> (g & 31)) & 1;
        }
        const bool st_vis = has && !(st & vis_mask);
        if (lmw::any(has && (!okg || st_vis != (id_v && !gone_v)))) { err = ST_UNSUPPORTED; break; }   // self-check (a)
        // ---- its element: the winners at A and V, where it stands and what it holds
        bool shows_a = false, shows_v = false, skew = false, bad = false, same_val = false, el_at_a = false;
        uint32_t v_lo = 0, v_hi = 0, l_lo = 0, l_hi = 0, v_blk = NONE, v_eid = NONE;
        if (id_v) {
          const uint32_t el = loc[g];
          const uint32_t ge = slot_of(el);
          if (ge == NONE) bad = true;
          else {
            const uint32_t sm = ml_ht_find(keys, cap, ml_key(el, false)), ss = ml_ht_find(keys, cap, ml_key(el, true));
            const unsigned long long mv = sm != NONE ? winV[sm] : 0ull, ma = sm != NONE ? winA[sm] : 0ull;
            const unsigned long long sv = ss != NONE ? winV[ss] : 0ull, sa = ss != NONE ? winA[ss] : 0ull;
            if ((sm != NONE && !mld_same(mv, best[sm])) || (ss != NONE && !mld_same(sv, best[ss]))) skew = true;   // self-check (b)
            const uint32_t pos_v = mv ? item_of(mv) : el;
            const uint32_t pos_a = ma ? item_of(ma) : (pid_ctr(el) < s_bA[pid_peer(el)] ? el : NONE);
            if ((mv && pos_v == NONE) || (ma && pos_a == NONE)) bad = true;
            shows_v = !gone_v && pos_v == pid;
            shows_a = id_a && !gone_a && pos_a == pid;
            if (pos_a != NONE && !bad) {
              const uint32_t ga = slot_of(pos_a);
              if (ga == NONE) bad = true; else el_at_a = !((bitA[ga >> 5] >> (ga & 31)) & 1);
            }
            if (!bad && shows_v) {
              // where the value at V (and, when the element shows at A, the value at A) lies: the winning set's, else the inserted one
              auto locate = [&](unsigned long long w, uint64_t& off, uint64_t& lim, uint32_t& blk, uint32_t& eid) {
                if (w) {
                  const uint32_t row = (uint32_t)((w - 1) & 0xffffffu);
                  if (row >= m.n_op) { bad = true; return; }
                  const OpRow wr = d.op[m.op0 + row];
                  blk = d.op_blk[m.op0 + row];
                  const BlockDesc& gb = d.blk[blk];
                  off = d.op_val[m.op0 + row];
                  lim = gb.base + gb.sec_rel[SEC_VALUES] + gb.sec_len[SEC_VALUES];
                  eid = pid_make(d.chg[wr.chg].peer, wr.ctr);
                } else { off = doc_data0 + d.cp[elem0 + ge]; lim = doc_end; blk = NONE; eid = el; }
                if (off >= lim) bad = true;
              };
              uint64_t off_v = 0, lim_v = 0;
              locate(sv, off_v, lim_v, v_blk, v_eid);
              v_lo = (uint32_t)off_v; v_hi = (uint32_t)(off_v >> 32); l_lo = (uint32_t)lim_v; l_hi = (uint32_t)(lim_v >> 32);
              if (el_at_a && !bad) {
                if (mld_same(sa, sv)) same_val = true;
                else {
                  uint64_t off_a = 0, lim_a = 0;
                  uint32_t blk_a, eid_a;
                  locate(sa, off_a, lim_a, blk_a, eid_a);
                  if (!bad) {
                    const uint32_t eq = md_value_eq(d.data + off_a, d.data + lim_a, d.data + off_v, d.data + lim_v);
                    if (eq == 1) same_val = true; else if (eq == 2) undecided |= 2u; else if (eq == 3) bad = true;
                  }
                }
              }
            }
          }
        }
        if (lmw::any(skew)) { err = ST_UNSUPPORTED; break; }
        if (lmw::any(bad)) { err = ST_DATA_CORRUPTION; break; }
        const uint64_t mK = lmw::ballot(shows_a && shows_v && same_val);
        const uint64_t mI = lmw::ballot(shows_v && !(shows_a && same_val));            // an R lane inserts …
        const uint64_t mD = lmw::ballot(shows_a && !(shows_v && same_val));            // … and deletes
        const uint64_t mF = lmw::ballot(shows_v && !shows_a && el_at_a && same_val);   // from_move
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
            retain += (uint32_t)lmw::popc64(mK & seg);
            continue;
          }
          if (!gap) {
            if (retain) { begin_op(); sink_lit(s, "{\"retain\":", 10); sink_i64(s, (int64_t)retain); sink_byte(s, '}'); retain = 0; }
            gap = true;
          }
          del += (uint32_t)lmw::popc64(mD & seg);
          for (uint64_t jm = mI & seg; jm && !err; jm &= jm - 1) {
            const int l = lmw::ffs64(jm);
            const bool flag = (mF >> l) & 1;
            if (ins_open && flag != ins_flag) close_ins();
            if (!ins_open) {
              begin_op();
              sink_lit(s, "{\"insert\":[", 11);
              ins_open = true; ins_flag = flag; first_item = true;
            }
            if (!first_item) sink_byte(s, ',');
            first_item = false;
            const uint64_t vabs = ((uint64_t)lmw::bcast(v_hi, l) << 32) | lmw::bcast(v_lo, l);
            const uint64_t vlim = ((uint64_t)lmw::bcast(l_hi, l) << 32) | lmw::bcast(l_lo, l);
            const uint32_t vblk = lmw::bcast(v_blk, l), eid = lmw::bcast(v_eid, l);
            Rd r = rd_make(d.data + vabs, vlim - vabs);
            if (*r.p == 9) {   // a child container: LoroValue::Container of the op that wrote it (the set, else the insert), never its content
              (void)rd_u8(r);
              const uint32_t child = rd_u8(r);
              sink_lit(s, "\"\xF0\x9F\xA6\x9C:cid:", 10);
              sink_i64(s, (int64_t)pid_ctr(eid));
              sink_byte(s, '@');
              sink_u64(s, pid_peer(eid) < m.n_peers ? d.peer_uniq[m.praw0 + pid_peer(eid)] : 0ull);
              if (child == CK_MAP) sink_lit(s, ":Map\"", 5);
              else if (child == CK_LIST) sink_lit(s, ":List\"", 6);
              else if (child == CK_TEXT) sink_lit(s, ":Text\"", 6);
              else if (child == CK_TREE) sink_lit(s, ":Tree\"", 6);
              else if (child == CK_MOVABLE) sink_lit(s, ":MovableList\"", 13);
              else if (child == CK_COUNTER) sink_lit(s, ":Counter\"", 9);
              else err = ST_UNSUPPORTED;
              continue;
            }
            sink_value(s, r, err, d, vblk, m.blk0, m.n_blk);
          }
        }
      }
    }
    if (gap) close_gap();
    if (cont_open) sink_byte(s, ']');
  }
  sink_byte(s, '}');
  if (s.pos > 0xfffffff0ull && !err) err = ST_UNSUPPORTED;
  undecided = lmw::any(undecided != 0) ? 2u : 0u;
  if (lane == 0) {
    res[q].status = err ? err : (int32_t)ST_OK;
    res[q].len = err ? 0u : (uint32_t)s.pos;   // (s.pos > s.cap: the host sees the size and launches again with room for it)
    res[q].cnt = n_listed;
    if (!err && undecided) res[q].other_changed |= undecided;
  }
}

}  // namespace lm
