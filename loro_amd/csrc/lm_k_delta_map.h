// Map deltas between two versions (include/loro_merge.h lm_delta_map): what LoroDoc::diff(a, b) and the MapDelta events of subscribe
// tell a subscriber about the Map containers, answered on the device from the LWW tables and op rows the last run left — kernels of
// their own behind lm_run, like k_delta: they read the document's key table (ht_key / ht_best / ht_list / ht_cnt), the op rows, the
// key rows and the value bytes, and write only their own winner words, sort scratch, slabs and result rows.
//
// A = the version the subscriber has (the query's from_vv), V = the version the run rendered.  Per (Map container, key) a WRITE is a
// Map set or Map delete row of an applied change beyond a sliced change's known prefix (k_map_lww's tests); the winner at a version X
// is the write with the greatest (lamport, peer) among the writes whose id lies in X (ctr < X[peer]); "no write in X" is a state of
// its own.  The run left the winner at V in best[slot], packed as (lamport, peer index, row) + 1; the winner at A is one more pass
// over the op rows.  A key is reported iff its two winners are different ops and (one of them is absent or a delete while the other
// is not, or both are sets whose values differ under LoroValue equality — diff_calc.rs:545-610, loro-common/src/value.rs:29-44).
//
// k_mdelta_mark lane = op row (dl_mark_row): a Map write row with ctr < V[peer] finds its key's slot in the document's table — by the
//               hash of the kernel that BUILT the table, restated below — and raises the query's winV[slot] (and winA[slot] when also
//               ctr < A[peer]) to the builders' packed word (dl_win_word, dl_win_raise).  A row whose key has no slot makes the query
//               LM_UNSUPPORTED.  Rows of MovableList / Tree / Counter containers with an id in V \ A set bit 0 of other_changed.
// k_mdelta      one wave per query, lanes over the claimed slots 64 per step.  SELF-CHECK: winV[slot] == best[slot] for every claimed
//               Map slot — the LWW builders against the op rows read again; a mismatch gives the query LM_UNSUPPORTED: the right
//               value or a refusal, never a guess.  The changed slots are compacted into the query's own list, bitonic-sorted by
//               (container, key bytes) and rendered container by container: {"updated":{…},"deleted":[…]}.  A pair of nested List
//               values or of nested Map values from different ops is not decided: the key is left out, bit 1 of other_changed is set.
// The query and result rows, the slabs and k_delta_pack are lm_k_delta.h's.
//
// The query's scratch (DlQuery: cap = the slots of the document's table, no bitmaps): winV[cap], winA[cap] (dl_win), then 64-bit key
// prefixes[cap], then the sort list of cap / 2 32-bit entries.
#pragma once
#include "lm_k_delta.h"

namespace lm {

// ---- the two hashes of the table builders, restated (k_mdelta's self-check catches a copy that drifts: a key then finds no slot or
// a slot whose winner differs)
// k_map_lww (lm_k_emit.h): fnv1a over the whole key, seeded with the container index
LM_DEV uint32_t md_hash_rows(const uint8_t* ks, uint32_t kl, uint32_t cidx) { return (uint32_t)fnv1a(ks, kl, 0xcbf29ce484222325ull ^ cidx); }
// k_map_lww_doc (lm_k_lww_doc.h): container, length and the first eight bytes mixed, fnv1a over the rest
LM_DEV uint32_t md_hash_doc(const uint8_t* ks, uint32_t kl, uint32_t cidx) {
  unsigned long long pf = 0;
  for (uint32_t q = 0; q < 8; q++) pf = (pf << 8) | (q < kl ? ks[q] : 0u);
  uint64_t h = (0xcbf29ce484222325ull ^ cidx ^ ((uint64_t)kl << 32)) * 0x100000001b3ull;
  h = (h ^ pf) * 0x9E3779B97F4A7C15ull;
  if (kl > 8) h = fnv1a(ks + 8, kl - 8, h);
  h ^= h >> 29;
  return (uint32_t)h;
}
// which builder left the document's table: k_map_lww_doc's documents are those of a batch whose table fits LDS, without a MovableList,
// that did not take the second pass (a DF_LWW_RETRY document's ht0 / ht_cap name the table k_map_lww filled for it)
LM_DEV bool md_doc_hash(uint32_t lds_on, uint32_t cap, uint32_t flags) {
  return lds_on && cap <= LWW_LDS_CAP && !(flags & (DF_MOVABLE | DF_LWW_RETRY));
}
// slot of (container, key row) in the document's table, NONE when the table does not hold the key.  MovableList entries (ml_key, bit
// 63) are never read as Map keys.
LM_DEV uint32_t md_find(const Dev& d, const unsigned long long* keys, uint32_t cap, uint32_t cidx, uint32_t krow, bool doc_hash) {
  if (!cap) return NONE;
  const uint8_t* ks = d.data + d.key_off[krow];
  const uint32_t kl = d.key_len[krow];
  uint32_t slot = (doc_hash ? md_hash_doc(ks, kl, cidx) : md_hash_rows(ks, kl, cidx)) & (cap - 1);
  for (uint32_t probe = 0; probe < cap; probe++, slot = (slot + 1) & (cap - 1)) {
    const unsigned long long cur = keys[slot];
    if (cur == HT_EMPTY) return NONE;
    if ((cur >> 63) || (uint32_t)(cur >> 32) != cidx) continue;
    const uint32_t orow = (uint32_t)cur;
    if (orow == krow || (d.key_len[orow] == kl && bytes_eq(d.data + d.key_off[orow], ks, kl))) return slot;
  }
  return NONE;
}

LM_KERNEL void k_mdelta_mark(Dev d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, uint32_t* scr, DlRes* res, uint32_t lds_on) {
  DlRow x;
  if (!dl_mark_row(d, qs, nq, bnd, x)) return;
  const OpRow& r = x.r;
  if (x.ck == CK_MOVABLE || x.ck == CK_TREE || x.ck == CK_COUNTER) {
    if (dl_other_changed(r, x.bA, x.bV)) lmw::atomic_or(&res[x.q].other_changed, 1u);
    return;
  }
  if (x.ck != CK_MAP || (x.kind != OK_MAP_SET && x.kind != OK_MAP_DEL)) return;
  if (!d.chg_flag[r.chg]) return;                              // not an applied change
  if (r.ctr < x.ch.ctr + d.chg_skip[r.chg]) return;            // already-known prefix of a sliced change
  if (r.ctr >= x.bV) return;                                   // beyond the rendered version: does not compete
  const unsigned long long v = dl_win_word(d, x);
  if (!v) { dl_refuse(res, x.q); return; }
  const uint32_t slot = md_find(d, d.ht_key + d.ht0[x.Q.doc], x.Q.cap, x.cidx, r.a0, md_doc_hash(lds_on, x.Q.cap, x.m.flags));
  if (slot == NONE) { dl_refuse(res, x.q); return; }
  dl_win_raise(dl_win(scr, x.Q) + slot, x.Q.cap, v, r.ctr < x.bA);
}

LM_KERNEL LM_ONE_WAVE_GROUPS void k_mdelta(Dev d, const DlQuery* qs, uint32_t* scr, uint8_t* out, const uint64_t* out_off, DlRes* res) {
  const uint32_t q = (uint32_t)lmw::bid();
  const int lane = lmw::lane();
  const DlQuery Q = qs[q];
  const uint32_t doc = Q.doc;
  const DocMeta m = d.doc[doc];
  if (status_fatal(m.status)) { dl_finish(res, q, m.status, 0, 0, 0); return; }
  int32_t err = res[q].status;   // (k_mdelta_mark: a write whose key the table does not hold)
  const uint32_t cap = Q.cap, list_cap = cap / 2;
  unsigned long long* winV = dl_win(scr, Q);
  const unsigned long long* winA = winV + cap;
  unsigned long long* pfx = winV + 2ull * cap;
  uint32_t* lst = (uint32_t*)(pfx + cap);
  const unsigned long long* keys = d.ht_key + d.ht0[doc];
  const unsigned long long* best = d.ht_best + d.ht0[doc];
  const uint32_t* claimed = d.ht_list + 2 * d.ht0[doc];
  uint32_t n_claimed = cap ? d.ht_cnt[doc] : 0u;
  if (cap != d.ht_cap[doc] || n_claimed > cap / 2) { err = err ? err : (int32_t)ST_UNSUPPORTED; n_claimed = 0; }
  // ---- classes, 64 claimed slots per step; the changed ones into the list
  uint32_t K = 0, undecided = 0;
  for (uint32_t c0 = 0; c0 < n_claimed && !err; c0 += 64) {
    const uint32_t ci = c0 + (uint32_t)lane;
    bool changed = false, bad = false, und = false, skew = false;
    uint32_t sl = 0;
    if (ci < n_claimed) {
      sl = claimed[ci];
      if (sl >= cap) bad = true;
      else {
        const unsigned long long k = keys[sl];
        if (!(k >> 63) && k != HT_EMPTY) {                     // (a MovableList entry is no Map key)
          const unsigned long long wv = winV[sl], wa = winA[sl];
          if (wv != best[sl]) skew = true;                     // the self-check
          else if (wv != 0 && wa != wv) {
            const uint32_t rv = dl_win_row(wv), ra = wa ? dl_win_row(wa) : 0u;
            if (rv >= m.n_op || ra >= m.n_op) bad = true;
            else {
              const bool del_v = ((d.op[m.op0 + rv].cidx_kind >> 16) & 0xff) == OK_MAP_DEL;
              if (wa == 0) changed = true;
              else {
                const bool del_a = ((d.op[m.op0 + ra].cidx_kind >> 16) & 0xff) == OK_MAP_DEL;
                if (del_a != del_v) changed = true;
                else if (!del_v) {
                  const BlockDesc& ba = d.blk[d.op_blk[m.op0 + ra]];
                  const BlockDesc& bv = d.blk[d.op_blk[m.op0 + rv]];
                  const uint32_t eq = md_value_eq(d.data + d.op_val[m.op0 + ra], d.data + ba.base + ba.sec_rel[SEC_VALUES] + ba.sec_len[SEC_VALUES],
                                                  d.data + d.op_val[m.op0 + rv], d.data + bv.base + bv.sec_rel[SEC_VALUES] + bv.sec_len[SEC_VALUES]);
                  if (eq == 0) changed = true; else if (eq == 2) und = true; else if (eq == 3) bad = true;
                }
              }
            }
          }
        }
      }
    }
    if (lmw::any(skew)) { err = ST_UNSUPPORTED; break; }
    if (lmw::any(bad)) { err = ST_DATA_CORRUPTION; break; }
    if (lmw::any(und)) undecided = 2u;
    const uint64_t cm = lmw::ballot(changed);
    const uint32_t at = K + (uint32_t)lmw::popc64(cm & ((1ull << lane) - 1));
    if (changed & (at < list_cap)) {
      lst[at] = sl;
      const uint32_t kr = (uint32_t)keys[sl];
      const uint8_t* kp = d.data + d.key_off[kr];
      const uint32_t kl = d.key_len[kr];
      unsigned long long pf = 0;
      for (uint32_t b8 = 0; b8 < 8; b8++) pf = (pf << 8) | (b8 < kl ? kp[b8] : 0u);
      pfx[sl] = pf;
    }
    K += (uint32_t)lmw::popc64(cm);
  }
  uint32_t Kp = 1;
  while (Kp < K) Kp <<= 1;
  if (!err && Kp > list_cap && K) err = ST_INTERNAL;
  lmw::mem_fence();
  lmw::block_sync();   // (the list and the prefixes are read by other lanes than those that wrote them)
  // ---- the list in (container, key) order: bitonic, the prefixes first and the strings on a tie (k_emit_any's sort)
  if (!err && K > 1) {
    for (uint32_t i = K + (uint32_t)lane; i < Kp; i += 64) lst[i] = NONE;   // padding sorts last
    lmw::mem_fence();
    lmw::block_sync();
    auto less = [&](uint32_t sa, uint32_t sb) -> bool {
      if (sa == NONE) return false;
      if (sb == NONE) return true;
      const unsigned long long ka = keys[sa], kb = keys[sb];
      if ((ka >> 32) != (kb >> 32)) return (ka >> 32) < (kb >> 32);
      const unsigned long long pa = pfx[sa], pb = pfx[sb];
      if (pa != pb) return pa < pb;
      const uint32_t ra = (uint32_t)ka, rb = (uint32_t)kb;
      return bytes_cmp(d.data + d.key_off[ra], d.key_len[ra], d.data + d.key_off[rb], d.key_len[rb]) < 0;
    };
    for (uint32_t k2 = 2; k2 <= Kp; k2 <<= 1) {
      for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
        for (uint32_t t0 = 0; t0 < Kp / 2; t0 += 64) {
          const uint32_t t = t0 + (uint32_t)lane;
          if (t < Kp / 2) {
            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
            const uint32_t x = lst[i], y = lst[p];
            const bool up = (i & k2) == 0;
            if (up ? less(y, x) : less(x, y)) { lst[i] = y; lst[p] = x; }
          }
        }
        lmw::mem_fence();
        lmw::block_sync();
      }
    }
  }
  // ---- rendering, container by container
  Sink s = dl_sink(out, out_off, q);
  uint32_t n_listed = 0;
  sink_byte(s, '{');
  uint32_t e = 0;
  while (e < K && !err) {
    const uint32_t cidx = (uint32_t)(keys[lst[e]] >> 32);
    uint32_t g1 = K;   // end of the container's entries
    for (uint32_t b0 = e; b0 < K; b0 += 64) {
      const uint32_t i = b0 + (uint32_t)lane;
      const uint64_t dm = lmw::ballot(i < K ? (uint32_t)(keys[lst[i < K ? i : e]] >> 32) != cidx : false);
      if (dm) { g1 = b0 + (uint32_t)lmw::ffs64(dm); break; }
    }
    if (cidx >= m.n_cont) { err = ST_INTERNAL; break; }
    const ContRow o = d.cont[m.cid0 + cidx];
    if (n_listed) sink_byte(s, ',');
    n_listed++;
    sink_cid_key(s, d, m, o, ":Map\":{\"updated\":{", 18);
    for (int pass = 0; pass < 2 && !err; pass++) {
      bool first = true;
      for (uint32_t b0 = e; b0 < g1 && !err; b0 += 64) {
        // the chain list -> slot -> winning row -> key / value location for 64 entries at once, one per lane (k_emit_any)
        const uint32_t i = b0 + (uint32_t)lane;
        const bool act = i < g1;
        uint32_t g_row = 0, g_blk = 0, g_klen = 0, g_koff_lo = 0, g_koff_hi = 0, g_voff_lo = 0, g_voff_hi = 0, g_lim_lo = 0, g_lim_hi = 0;
        bool is_del = false;
        if (act) {
          const uint32_t sl = lst[i];
          const uint32_t krow = (uint32_t)keys[sl];
          g_row = m.op0 + dl_win_row(winV[sl]);
          is_del = ((d.op[g_row].cidx_kind >> 16) & 0xff) == OK_MAP_DEL;
          const uint64_t ko = d.key_off[krow];
          g_koff_lo = (uint32_t)ko; g_koff_hi = (uint32_t)(ko >> 32); g_klen = d.key_len[krow];
          g_blk = d.op_blk[g_row];
          const BlockDesc& gb = d.blk[g_blk];
          const uint64_t lim_o = gb.base + gb.sec_rel[SEC_VALUES] + gb.sec_len[SEC_VALUES], vo = d.op_val[g_row];
          g_lim_lo = (uint32_t)lim_o; g_lim_hi = (uint32_t)(lim_o >> 32); g_voff_lo = (uint32_t)vo; g_voff_hi = (uint32_t)(vo >> 32);
        }
        for (uint64_t jm = lmw::ballot(act & (is_del == (pass == 1))); jm && !err; jm &= jm - 1) {
          const int l = lmw::ffs64(jm);
          const uint64_t koff = ((uint64_t)lmw::bcast(g_koff_hi, l) << 32) | lmw::bcast(g_koff_lo, l);
          if (!first) sink_byte(s, ',');
          first = false;
          sink_string(s, d.data + koff, lmw::bcast(g_klen, l));
          if (pass) continue;
          sink_byte(s, ':');
          const uint32_t row = lmw::bcast(g_row, l), vblk = lmw::bcast(g_blk, l);
          const uint64_t voff = ((uint64_t)lmw::bcast(g_voff_hi, l) << 32) | lmw::bcast(g_voff_lo, l);
          const uint64_t limo = ((uint64_t)lmw::bcast(g_lim_hi, l) << 32) | lmw::bcast(g_lim_lo, l);
          if (voff >= limo) { err = ST_DATA_CORRUPTION; break; }
          Rd r = rd_make(d.data + voff, limo - voff);
          uint32_t child;
          if (rd_child(r, child)) {   // a child container created by the winning set
            const OpRow wr = d.op[row];
            sink_child_cid(s, d, m, d.chg[wr.chg].peer, wr.ctr, child, err);
            continue;
          }
          sink_value(s, r, err, d, vblk, m.blk0, m.n_blk);
        }
      }
      if (pass == 0) sink_lit(s, "},\"deleted\":[", 13);
    }
    sink_lit(s, "]}", 2);
    e = g1;
  }
  sink_byte(s, '}');
  dl_finish(res, q, err, s.pos, n_listed, undecided);
}

}  // namespace lm
