// Text deltas with style attributes between two versions (include/loro_merge.h lm_delta_richtext): what lm_delta tells about the
// scalars of a Text container, plus what a subscriber standing at A must do to the STYLES it holds — the call is to lm_delta what
// lm_richtext is to lm_fetch.  Kernels of their own behind lm_run, like k_delta: they read tracker memory, cp[] / tb[], the op rows and
// the style values, and write only the query's bitmaps, slabs and result rows — cp[] in particular is left alone (k_richtext parks
// CP_ALIVE marks there and takes them off again; here an anchor's facts are worked out from the query's own bitmaps where it stands).
//
// A = the query's from_vv, V = the version the run rendered; scalars are classed K / I / D exactly as k_delta classes them (lm_k_delta.h)
// and anchors are never elements of a delta.  A MARK is a StyleStart anchor (p, c) with its StyleEnd (p, c + 1), carrying the StyleOp
// (key, value, lamport, peer) of the Start row; it is live at A iff both anchors are in A by lm_delta's test (counter below A[p], no
// delete atom in A targets the slot) and live at V iff both are visible — which the self-check pins to the same test against V.
// attrs_X(s): per key the mark live at X with the greatest (lamport, peer) among those whose Start stands in front of s and whose End
// stands behind it; a null value removes the key.  An I scalar carries attrs_V, a D scalar nothing, a K scalar its CHANGE SET: key:
// attrs_V[key] where attrs_A lacks the key or holds an unequal value (LoroValue equality, md_value_eq), key: null where attrs_A has a
// key attrs_V lacks; the same op winning at A and at V changes nothing and compares nothing.  Runs are lm_delta's, also cut by
// attributes: neighbouring K scalars are one retain iff their change sets are equal (a joined run keeps the set it was opened with),
// the I scalars of a gap give one insert per maximal run of equal attrs_V, then at most one delete; a trailing retain is dropped only
// when it carries no attributes.  Two nested List / Map values of DIFFERENT ops are not compared (the family's rule, bit 1 of
// other_changed): the key counts as changed, the runs stay apart — a correct delta, only not a minimal one.
//
// k_rtdelta_mark lane = op row (dl_mark_row): a delete row of a Text container sets its targets' bits in gone-at-A / gone-at-V
//                (dl_mark_delete — the bitmaps cover anchor slots); a row of ANY other kind of container, List included, with an id
//                in V \ A raises bit 0 of other_changed.
// k_rtdelta      one wave per query, dl_open / dl_walk_all, both tracker layouts.  Per 64-element chunk: classes by ballot and
//                k_delta's self-check; the chunk is handled in the pieces between its anchors.  An anchor opens / closes its StyleOp
//                in TWO active sets in LDS (k_richtext's layout, once for A and once for V); keys are numbered per container as
//                they turn up and LANE k OWNS KEY k: after a change of a set and before the next scalar that needs them, every
//                entry finds out whether another one of its key beats it (n_act broadcast reads), the winners are scattered by key
//                number, and lane k forms the key's entry of attrs_V (for inserts) and of the change set (for retains) in registers
//                — 0 absent, 1 null, 2 + StyleStart row.  The open retain's and the open insert's sets are registers of the same
//                shape, so "equal change sets" is one ballot and, for the keys whose rows differ, a value comparison per lane.
//                The carry across chunks and leaves is k_delta's plus those two sets.  Attribute keys are written in bytewise
//                order with the renderer's escapes, values with sink_value, inserts by all lanes at once (cp_bytes + sink_lanes).
// Output: optimistic slabs, exact sizes, a second launch on overflow, k_delta_pack — Engine::delta_run.
// Limits: RT_MAX marks live at one place at A or at V and RT_MAX distinct keys per Text (LM_UNSUPPORTED beyond), as k_richtext.
#pragma once
#include "lm_k_delta.h"

namespace lm {

struct DrSets {            // [0] = A, [1] = V
  uint32_t act[2][RT_MAX];   // StyleStart rows (inside the document) of the open StyleOps
  uint32_t lam[2][RT_MAX];   // … their lamports,
  uint32_t pk[2][RT_MAX];    // … peer | null value << 31
  uint32_t kid[2][RT_MAX];   // … and key numbers
  uint32_t win[2][RT_MAX];   // per key number: the winner's entry — 0 none, 1 a null value, 2 + StyleStart row
  unsigned long long kp[RT_MAX];   // the keys of this container, numbered as they turn up
  uint32_t kl[RT_MAX];
};

// two entries of one key (0 absent, 1 null, 2 + StyleStart row), one pair per lane: 1 equal, 0 not, 2 two nested values of different
// ops (not compared here), 3 damaged
LM_DEV uint32_t dr_entry_eq(const Dev& d, const DocMeta& m, uint32_t a, uint32_t b) {
  if (a == b) return 1;
  if (a < 2 || b < 2) return 0;
  int32_t e = 0;
  const RtStyle A = rt_style(d, m, a - 2, e), B = rt_style(d, m, b - 2, e);
  if (e || !A.vl || !B.vl) return 3;
  return md_value_eq(A.vp, A.vp + A.vl, B.vp, B.vp + B.vl);
}

LM_KERNEL void k_rtdelta_mark(Dev d, const DlQuery* qs, uint32_t nq, const uint32_t* bnd, uint32_t* scr, DlRes* res) {
  DlRow x;
  if (!dl_mark_row(d, qs, nq, bnd, x)) return;
  if (x.ck != CK_TEXT) {
    if (dl_other_changed(x.r, x.bA, x.bV)) lmw::atomic_or(&res[x.q].other_changed, 1u);
    return;
  }
  if (x.kind == OK_DEL) dl_mark_delete(d, x, dl_bits(scr, x.Q), res);
}

LM_KERNEL LM_ONE_WAVE_GROUPS void k_rtdelta(Dev d, const DlQuery* qs, const uint32_t* bnd, uint32_t* scr, uint8_t* out, const uint64_t* out_off, DlRes* res, int units) {
  static_assert(RT_MAX == 64 && RT_BLOCK == 64, "lane k owns key k; the LDS tables belong to a single wave");
  const uint32_t q = (uint32_t)lmw::bid();
  const int lane = lmw::lane();
  const DlQuery Q = qs[q];
  const DocMeta m = d.doc[Q.doc];
  if (status_fatal(m.status)) { dl_finish(res, q, m.status, 0, 0, 0); return; }
  LM_SHARED(DlLds, s_lds, 1);
  LM_SHARED(DrSets, s_sets, 1);
  DlLds& L = s_lds[0];
  DrSets& S = s_sets[0];
  const DlDoc D = dl_open(d, Q, m, bnd, L);
  const uint32_t* bitA = dl_bits(scr, Q);
  const uint32_t* bitV = bitA + Q.n_words;
  Sink s = dl_sink(out, out_off, q);
  int32_t err = res[q].status;   // (k_rtdelta_mark: a delete's targets lie beyond the document's element slots)
  uint32_t n_listed = 0, undecided = 0;
  sink_byte(s, '{');
  for (uint32_t cidx = 0; cidx < m.n_cont && !err; cidx++) {
    const ContRow o = d.cont[m.cid0 + cidx];
    if ((o.kind_root & 0xff) != CK_TEXT) continue;
    // ---- the carry: wave-uniform, across chunks and leaves — k_delta's, plus the sets of the open retain and the open insert
    uint32_t retain = 0, del = 0;
    bool gap = false, ins_open = false, cont_open = false;
    uint32_t n_a = 0, n_v = 0, n_keys = 0;                 // open StyleOps at A and at V; keys numbered so far
    bool dirty_w = false, dirty_k = false, dirty_i = false;
    uint32_t wA = 0, wV = 0;                              // lane k: the winners of key k at A and at V
    uint32_t cur_k = 0, cur_i = 0, open_r = 0, open_i = 0;   // lane k: key k's entry of the change set / of attrs_V, now and when the run was opened
    auto begin_op = [&]() {
      if (cont_open) { sink_byte(s, ','); return; }
      if (n_listed) sink_byte(s, ',');
      n_listed++;
      cont_open = true;
      sink_cid_key(s, d, m, o, ":Text\":[", 8);
    };
    auto winners = [&]() {
      lmw::block_sync();
      S.win[0][lane] = 0; S.win[1][lane] = 0;
      lmw::block_sync();
      for (int x = 0; x < 2; x++) {
        const uint32_t n = x ? n_v : n_a;
        const bool mine = (uint32_t)lane < n;
        const uint32_t kid = mine ? S.kid[x][lane] : 0u, lam = mine ? S.lam[x][lane] : 0u, pk = mine ? S.pk[x][lane] : 0u;
        bool beaten = false;
        for (uint32_t j = 0; j < n; j++) {
          const uint32_t jl = S.lam[x][j], jp = S.pk[x][j] & 0x7fffffffu;
          beaten |= S.kid[x][j] == kid && (jl > lam || (jl == lam && jp > (pk & 0x7fffffffu)));
        }
        if (mine && !beaten) S.win[x][kid] = (pk >> 31) ? 1u : 2u + S.act[x][lane];
      }
      lmw::block_sync();
      wA = S.win[0][lane]; wV = S.win[1][lane];
      dirty_w = false;
    };
    auto form_k = [&]() {   // the change set of a K scalar
      if (dirty_w) winners();
      cur_k = 0;
      uint32_t bad = 1;
      const bool pa = wA >= 2, pv = wV >= 2;
      if (pv && !pa) cur_k = wV;
      else if (pa && !pv) cur_k = 1;
      else if (pa && pv && wA != wV) {
        bad = dr_entry_eq(d, m, wA, wV);
        if (bad != 1) cur_k = wV;
        if (bad == 2) undecided = 1;
      }
      if (lmw::any(bad == 3)) err = err ? err : (int32_t)ST_DATA_CORRUPTION;
      dirty_k = false;
    };
    auto form_i = [&]() {   // attrs_V of an I scalar
      if (dirty_w) winners();
      cur_i = wV >= 2 ? wV : 0u;
      dirty_i = false;
    };
    auto differs = [&](uint32_t a, uint32_t b) -> bool {   // two sets, lane k holding key k's entries
      if (!lmw::any(a != b)) return false;
      const uint32_t r = dr_entry_eq(d, m, a, b);
      if (r == 2) undecided = 1;
      if (lmw::any(r == 3)) err = err ? err : (int32_t)ST_DATA_CORRUPTION;
      return lmw::any(r != 1);
    };
    auto write_attrs = [&](uint32_t ent) {   // "attributes":{…}, — nothing for an empty set
      uint64_t todo = lmw::ballot(ent != 0);
      if (!todo) return;
      sink_lit(s, "\"attributes\":{", 14);
      bool first = true;
      while (todo && !err) {
        int best = lmw::ffs64(todo);   // the bytewise smallest key not yet written
        for (uint64_t r = todo & (todo - 1); r; r &= r - 1) {
          const int j = lmw::ffs64(r);
          if (bytes_cmp((const uint8_t*)(uintptr_t)S.kp[j], S.kl[j], (const uint8_t*)(uintptr_t)S.kp[best], S.kl[best]) < 0) best = j;
        }
        todo &= ~(1ull << best);
        if (!first) sink_byte(s, ',');
        first = false;
        sink_string(s, (const uint8_t*)(uintptr_t)S.kp[best], S.kl[best]);
        sink_byte(s, ':');
        const uint32_t e = lmw::bcast(ent, best);
        if (e == 1) sink_lit(s, "null", 4);
        else {
          const RtStyle W = rt_style(d, m, e - 2, err);
          Rd vr = rd_make(W.vp, W.vl);
          sink_value(s, vr, err, d, W.blk, m.blk0, m.n_blk);
        }
      }
      sink_lit(s, "},", 2);
    };
    auto emit_retain = [&]() {
      begin_op();
      sink_byte(s, '{');
      write_attrs(open_r);
      sink_lit(s, "\"retain\":", 9);
      sink_i64(s, (int64_t)retain);
      sink_byte(s, '}');
      retain = 0;
    };
    auto close_gap = [&]() {
      if (ins_open) { sink_lit(s, "\"}", 2); ins_open = false; }
      if (del) { begin_op(); sink_lit(s, "{\"delete\":", 10); sink_i64(s, (int64_t)del); sink_byte(s, '}'); del = 0; }
      gap = false;
    };
    dl_walk_all(d, m, cidx, D.P, L, [&](bool has, uint32_t pid, uint32_t g, uint32_t st) -> bool {
      // ---- classes (k_delta's, the self-check included)
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
      bool anc = false;
      if (in_a || in_v) {
        if (d.span) {
          const uint32_t t = d.tb[D.elem0 + g];
          anc = t == TB_ANCHOR;
          cpv = (t == TB_WIDE || anc) ? d.cp[D.elem0 + g] : t;
        } else { cpv = d.cp[D.elem0 + g]; anc = cpv >= CP_ANCHOR; }
      }
      const uint64_t ancA = lmw::ballot(anc && in_a), ancV = lmw::ballot(anc && in_v);
      uint64_t am = ancA | ancV;
      if (anc) { in_a = false; in_v = false; }
      const uint64_t mK = lmw::ballot(in_a && in_v), mI = lmw::ballot(!in_a && in_v), mD = lmw::ballot(in_a && !in_v);
      const uint64_t mW = units == 1 ? lmw::ballot((in_a || in_v) && cpv >= 0x10000u) : 0ull;   // one UTF-16 unit more
      uint32_t lo = 0;
      for (;;) {
        const uint32_t a = am ? (uint32_t)lmw::ffs64(am) : 64u;
        const uint64_t piece = (a >= 64 ? ~0ull : (1ull << a) - 1) & ~(lo >= 64 ? ~0ull : (1ull << lo) - 1);
        if ((mK | mI | mD) & piece)
          dl_segments(mK & piece, mI & piece, mD & piece, [&](bool is_k, uint64_t seg) -> bool {
            seg &= piece;
            if (is_k) {
              if (gap) close_gap();
              if (dirty_k) form_k();
              if (retain && differs(open_r, cur_k)) emit_retain();
              if (!retain) open_r = cur_k;
              retain += (uint32_t)lmw::popc64(mK & seg) + (uint32_t)lmw::popc64(mK & mW & seg);
              return !err;
            }
            if (!gap) {
              if (retain) emit_retain();
              gap = true;
            }
            del += (uint32_t)lmw::popc64(mD & seg) + (uint32_t)lmw::popc64(mD & mW & seg);
            const uint64_t im = mI & seg;
            if (!im) return true;
            if (dirty_i) form_i();
            if (ins_open && differs(open_i, cur_i)) { sink_lit(s, "\"}", 2); ins_open = false; }
            if (!ins_open) {
              begin_op();
              sink_byte(s, '{');
              open_i = cur_i;
              write_attrs(open_i);
              sink_lit(s, "\"insert\":\"", 10);
              ins_open = true;
            }
            uint64_t bytes = 0;
            uint32_t nb = 0;
            if ((im >> lane) & 1) cp_bytes(cpv, bytes, nb);
            sink_lanes(s, bytes, nb);
            return !err;
          });
        if (a >= 64 || err) break;
        // ---- the anchor in lane a
        const uint32_t av = lmw::bcast(cpv, (int)a), ag = lmw::bcast(g, (int)a), aid = lmw::bcast(pid, (int)a);
        const uint32_t rrel = av & ~(CP_ANCHOR | CP_ALIVE);
        if (rrel >= m.n_op) { err = ST_INTERNAL; break; }
        const OpRow r = d.op[m.op0 + rrel];
        const uint32_t kind = (r.cidx_kind >> 16) & 0xff;
        if (kind == OK_STYLE_START) {
          // its End is the next id of the same peer, one slot on (every writer emits the pair)
          const uint32_t ape = pid_peer(aid), actr = pid_ctr(aid), ge = ag + 1;
          bool pair = ge < Q.n_bits && r.ctr + 2 <= d.peer_ext[m.praw0 + ape] && d.cp[D.elem0 + ge] == (CP_ANCHOR | (rrel + 1));
          if (pair && d.span) pair = d.tb[D.elem0 + ge] == TB_ANCHOR;
          bool live_a = false, live_v = false;
          if (pair) {
            const uint32_t wa = bitA[ge >> 5], wv = bitV[ge >> 5];
            live_a = ((ancA >> a) & 1) && actr + 1 < L.bA[ape] && !((wa >> (ge & 31)) & 1);
            live_v = ((ancV >> a) & 1) && actr + 1 < L.bV[ape] && !((wv >> (ge & 31)) & 1);
          }
          if (live_a || live_v) {
            const RtStyle A = rt_style(d, m, rrel, err);
            const bool hit = (uint32_t)lane < n_keys && S.kl[lane] == A.kl &&
                             (S.kp[lane] == (unsigned long long)(uintptr_t)A.kp || bytes_eq((const uint8_t*)(uintptr_t)S.kp[lane], A.kp, A.kl));
            const uint64_t hm = lmw::ballot(hit);
            uint32_t kid = hm ? (uint32_t)lmw::ffs64(hm) : NONE;
            if (kid == NONE && n_keys < RT_MAX) {
              lmw::block_sync();
              if (lane == 0) { S.kp[n_keys] = (unsigned long long)(uintptr_t)A.kp; S.kl[n_keys] = A.kl; }
              lmw::block_sync();
              kid = n_keys++;
            }
            if (kid == NONE || (live_a && n_a >= RT_MAX) || (live_v && n_v >= RT_MAX)) err = err ? err : (int32_t)ST_UNSUPPORTED;
            else {
              lmw::block_sync();
              if (lane < 2 && (lane ? live_v : live_a)) {
                const uint32_t x = (uint32_t)lane, n = lane ? n_v : n_a;
                S.act[x][n] = rrel; S.lam[x][n] = A.lam; S.pk[x][n] = A.peer | (A.null ? 0x80000000u : 0u); S.kid[x][n] = kid;
              }
              lmw::block_sync();
              n_a += live_a ? 1u : 0u; n_v += live_v ? 1u : 0u;
              dirty_w = dirty_k = dirty_i = true;
            }
          }
        } else if (kind == OK_STYLE_END && rrel > 0) {
          for (uint32_t x = 0; x < 2; x++) {
            const uint32_t n = x ? n_v : n_a;
            const uint64_t fm = lmw::ballot((uint32_t)lane < n && S.act[x][lane] == rrel - 1);
            if (!fm) continue;
            const uint32_t i = (uint32_t)lmw::ffs64(fm), l = n - 1;
            const uint32_t v0 = S.act[x][l], v1 = S.lam[x][l], v2 = S.pk[x][l], v3 = S.kid[x][l];
            lmw::block_sync();
            if (lane == 0) { S.act[x][i] = v0; S.lam[x][i] = v1; S.pk[x][i] = v2; S.kid[x][i] = v3; }
            lmw::block_sync();
            if (x) n_v--; else n_a--;
            dirty_w = dirty_k = dirty_i = true;
          }
        }
        if (err) break;
        am &= am - 1;
        lo = a + 1;
      }
      return !err;
    });
    if (gap) close_gap();
    else if (retain && !err && lmw::any(open_r != 0)) emit_retain();   // a trailing retain stays only with attributes
    if (cont_open) sink_byte(s, ']');
  }
  sink_byte(s, '}');
  dl_finish(res, q, err, s.pos, n_listed, undecided);
}

}  // namespace lm
