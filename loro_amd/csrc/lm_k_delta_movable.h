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
// k_mldelta_mark lane = op row (dl_mark_row).  Rows of MovableList containers: a delete row sets its targets' bits in the gone-at-A /
//                gone-at-V bitmaps (dl_mark_delete); a move row sets the bit of the item it took the element from (the integrate kernels
//                left its id in the move item's cp[] slot) and raises the element's move winner; a set row raises its set winner.
//                Winner words are indexed by the slot the element's key (ml_key) has in the document's table and raised to
//                k_mlist_post's packed word (dl_win_word, dl_win_raise) — winV for rows below V, winA for rows below A.  Duplicate
//                blobs are idempotent: the same (lamport, peer) from another row.  Rows of Tree / Counter containers with an id in
//                V \ A set bit 0.
// k_mldelta      one wave per query; per MovableList container every item in sequence order (dl_walk_all).  SELF-CHECK, the right value
//                or a refusal (LM_UNSUPPORTED):
//                (a) for every item "visible by status word" == "id below V and bit V clear";
//                (b) for every element of an item in V the move and set winners at V raised from the op rows name the ops the run
//                    left in the document's table (compared without the row index: a duplicated blob holds the op in two rows).
//                Classes by ballots, k_delta's wave-uniform carry, values through the emitter's sink.
// The query and result rows, the scratch layout (DlQuery: winner words over the cap slots of the document's table, then the two bitmaps),
// the slabs and k_delta_pack are lm_k_delta.h's.
#pragma once
#include "lm_k_delta_map.h"

namespace lm {

// two packed winner words name the same op (or both name none): the row index in the low 24 bits is left out
LM_DEV bool mld_same(unsigned long long a, unsigned long long b) {
  if (a == 0 || b == 0) return a == b;
  return ((a - 1) >> 24) == ((b - 1) >> 24);
}

LM_KERNEL void k_mldelta_mark(Dev d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, uint32_t* scr, DlRes* res) {
  DlRow x;
  if (!dl_mark_row(d, qs, nq, bnd, x)) return;
  const OpRow& r = x.r;
  const DlQuery& Q = x.Q;
  const DocMeta& m = x.m;
  if (x.ck == CK_TREE || x.ck == CK_COUNTER) {
    if (dl_other_changed(r, x.bA, x.bV)) lmw::atomic_or(&res[x.q].other_changed, 1u);
    return;
  }
  if (x.ck != CK_MOVABLE) return;
  uint32_t* bits = dl_bits(scr, Q);
  if (x.kind == OK_DEL) { dl_mark_delete(d, x, bits, res); return; }
  if (x.kind != OK_LIST_MOVE && x.kind != OK_LIST_SET) return;
  if (r.ctr >= x.bV) return;                            // beyond the rendered version: does not compete
  const unsigned long long v = dl_win_word(d, x);
  if (!v) { dl_refuse(res, x.q); return; }
  const uint32_t pid_e = ml_resolve(d, m, x.cidx, r.a0, r.a1);
  if (pid_e == NONE) { dl_refuse(res, x.q); return; }
  if (x.kind == OK_LIST_MOVE) {                         // the item the move took the element from (lm_k_integrate*.h: the move item's cp[] slot)
    const uint64_t gm = (uint64_t)d.elem_base[m.praw0 + x.peer] + r.ctr;
    if (gm >= Q.n_bits || gm >= m.atoms) { dl_refuse(res, x.q); return; }
    const uint32_t tgt = (d.cp + (((uint64_t)m.elem0_hi << 32) | m.elem0_lo))[gm];
    if (tgt == NONE || pid_peer(tgt) >= Q.n_bnd) { dl_refuse(res, x.q); return; }
    const uint64_t gt = (uint64_t)d.elem_base[m.praw0 + pid_peer(tgt)] + pid_ctr(tgt);   // gone at V and, for a move below A, at A
    bool ok = dl_mark_range(bits + Q.n_words, Q.n_bits, gt, gt + 1);
    if (r.ctr < x.bA) ok &= dl_mark_range(bits, Q.n_bits, gt, gt + 1);
    if (!ok) dl_refuse(res, x.q);
  }
  const uint32_t slot = ml_ht_find(d.ht_key + d.ht0[Q.doc], Q.cap, ml_key(pid_e, x.kind == OK_LIST_SET));
  if (slot == NONE) { dl_refuse(res, x.q); return; }
  dl_win_raise(dl_win(scr, Q) + slot, Q.cap, v, r.ctr < x.bA);
}

LM_KERNEL LM_ONE_WAVE_GROUPS void k_mldelta(Dev d, const DlQuery* qs, const uint32_t* bnd, uint32_t* scr, uint8_t* out, const uint64_t* out_off, DlRes* res) {
  const uint32_t q = (uint32_t)lmw::bid();
  const DlQuery Q = qs[q];
  const uint32_t doc = Q.doc;
  const DocMeta m = d.doc[doc];
  if (status_fatal(m.status)) { dl_finish(res, q, m.status, 0, 0, 0); return; }
  LM_SHARED(DlLds, s_lds, 1);
  DlLds& L = s_lds[0];
  const DlDoc D = dl_open(d, Q, m, bnd, L);
  const uint32_t P = D.P, cap = Q.cap;
  const uint64_t elem0 = D.elem0;
  const unsigned long long* winV = dl_win(scr, Q);
  const unsigned long long* winA = winV + cap;
  const uint32_t* bitA = dl_bits(scr, Q);
  const uint32_t* bitV = bitA + Q.n_words;
  const unsigned long long* keys = d.ht_key + d.ht0[doc];
  const unsigned long long* best = d.ht_best + d.ht0[doc];
  const uint32_t* loc = d.loc + elem0;
  Sink s = dl_sink(out, out_off, q);
  int32_t err = res[q].status;   // (k_mldelta_mark: a target beyond the element slots, a key the table does not hold)
  if (!err && cap != d.ht_cap[doc]) err = ST_UNSUPPORTED;
  uint32_t n_listed = 0, undecided = 0;
  // slot of an item id, NONE when it lies beyond the bitmaps
  auto slot_of = [&](uint32_t id) -> uint32_t {
    if (id == NONE || pid_peer(id) >= P) return NONE;
    const uint64_t g = (uint64_t)L.eb[pid_peer(id)] + pid_ctr(id);
    return g < Q.n_bits && g < m.atoms ? (uint32_t)g : NONE;
  };
  // the item a packed move winner placed
  auto item_of = [&](unsigned long long w) -> uint32_t {
    const uint32_t row = dl_win_row(w);
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
      sink_cid_key(s, d, m, o, ":MovableList\":[", 15);
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
    dl_walk_all(d, m, cidx, P, L, [&](bool has, uint32_t pid, uint32_t g, uint32_t st) -> bool {
      // ---- the item: in A / in V by id, gone at A / at V by the bitmaps
      const uint32_t pe = pid_peer(pid), ct = pid_ctr(pid);
      const bool okg = has && pe < P && g < Q.n_bits && g < m.atoms;
      bool id_a = false, id_v = false, gone_a = false, gone_v = false;
      if (okg) {
        id_a = ct < L.bA[pe]; id_v = ct < L.bV[pe];
        gone_a = (bitA[g >> 5] >> (g & 31)) & 1; gone_v = (bitV[g >> 5] >> (g & 31)) & 1;
      }
      const bool st_vis = has && !(st & D.vis_mask);
      if (lmw::any(has && (!okg || st_vis != (id_v && !gone_v)))) { err = ST_UNSUPPORTED; return false; }   // self-check (a)
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
          const uint32_t pos_a = ma ? item_of(ma) : (pid_ctr(el) < L.bA[pid_peer(el)] ? el : NONE);
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
                const uint32_t row = dl_win_row(w);
                if (row >= m.n_op) { bad = true; return; }
                const OpRow wr = d.op[m.op0 + row];
                blk = d.op_blk[m.op0 + row];
                const BlockDesc& gb = d.blk[blk];
                off = d.op_val[m.op0 + row];
                lim = gb.base + gb.sec_rel[SEC_VALUES] + gb.sec_len[SEC_VALUES];
                eid = pid_make(d.chg[wr.chg].peer, wr.ctr);
              } else { off = D.data0 + d.cp[elem0 + ge]; lim = D.end; blk = NONE; eid = el; }
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
      if (lmw::any(skew)) { err = ST_UNSUPPORTED; return false; }
      if (lmw::any(bad)) { err = ST_DATA_CORRUPTION; return false; }
      const uint64_t mK = lmw::ballot(shows_a && shows_v && same_val);
      const uint64_t mI = lmw::ballot(shows_v && !(shows_a && same_val));            // an R lane inserts …
      const uint64_t mD = lmw::ballot(shows_a && !(shows_v && same_val));            // … and deletes
      const uint64_t mF = lmw::ballot(shows_v && !shows_a && el_at_a && same_val);   // from_move
      dl_segments(mK, mI, mD, [&](bool is_k, uint64_t seg) -> bool {
        if (is_k) {
          if (gap) close_gap();
          retain += (uint32_t)lmw::popc64(mK & seg);
          return true;
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
          uint32_t child;
          if (rd_child(r, child)) sink_child_cid(s, d, m, pid_peer(eid), pid_ctr(eid), child, err);   // named by the op that wrote it: the set, else the insert
          else sink_value(s, r, err, d, vblk, m.blk0, m.n_blk);
        }
        return !err;
      });
      return !err;
    });
    if (gap) close_gap();
    if (cont_open) sink_byte(s, ']');
  }
  sink_byte(s, '}');
  dl_finish(res, q, err, s.pos, n_listed, undecided);
}

}  // namespace lm
