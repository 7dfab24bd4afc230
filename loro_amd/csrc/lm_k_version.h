// Frontiers and version vectors (include/loro_merge.h lm_frontiers / lm_versions): the reference's conversions and comparisons —
// AppDag::frontiers_to_vv (oplog/loro_dag.rs:1192-1207), vv_to_frontiers / shrink_frontiers (:1269-1298), cmp_frontiers (:1347-1355),
// cmp_with_frontiers (:1333-1341), oplog_frontiers / state_frontiers (loro.rs:1377-1384) — answered on the device from the tables the
// DAG stage of the last run left behind: the version vector at the head of every DAG node (d.vvh), the change -> node map
// (g.chg_node), find_change and the sorted peer table.  A kernel of its own behind lm_run, like k_cursor: it reads those tables and
// writes only its own result rows.  The host parses the query bytes into (PeerID, counter) rows (Engine::versions), no byte is parsed here.
//
// Everything is evaluated over the APPLIED history of the document, whatever version the run rendered: a peer's applied end is
// peer_end_all where k_dag_b wrote it (resident documents, a batch entry with a checkout) and peer_end otherwise (a batch entry at its
// latest version: k_dag_b leaves peer_end_all alone there).  Pending changes are not part of it — find_change knows applied changes only.
//
// By id sets: closure(id) = the id and its causal past; heads(S) = the ids of S no other id of S has in its past.
//   closure vector of (q, c): vvh[node(q, c)][p] for p != q — a node's changes past its head depend on their own peer only — and
//   max(vvh[node][q], c + 1) for p == q: the id may stand in the middle of the node.
//   heads of a set of ids: the ids of one peer are a chain, so a peer's candidate is its greatest id; the candidate of p is dropped
//   iff for some candidate (q, c), q != p, the closure vector of (q, c) holds it: vvh[node(q, c)][p] > p's counter.
// One wave per query.  The ids are resolved 64 at a time (lane = id: binary search over peer_uniq, find_change, chg_node), then every
// resolved id is broadcast and the closure vector accumulated with lane = peer in strides of 64, in LDS.  The heads: lanes run over p,
// a loop over the candidates q, the survivors compacted by ballot — up to 255 x 255 word loads, coalesced along p, no serial walk.
#pragma once
#include "lm_k_lca.h"

namespace lm {

// == LM_VER_* in include/loro_merge.h; VER_HEADS is lm_frontiers' (b0 = which)
enum : int32_t { VER_TO_VV = 0, VER_TO_FRONTIERS = 1, VER_MINIMIZE = 2, VER_CMP = 3, VER_CMP_DOC = 4, VER_HEADS = 5 };
enum : int32_t { VER_LESS = -1, VER_EQUAL = 0, VER_GREATER = 1, VER_CONCURRENT = 2 };

struct VerId { uint64_t peer; uint32_t ctr; uint32_t neg; };   // neg: the counter is negative (no id has one)
struct VerQuery {
  uint32_t doc; int32_t op;
  uint32_t a0, na, b0, nb;   // rows [a0, a0 + na) and [b0, b0 + nb) of the call's id rows (VER_HEADS: b0 = which)
  uint64_t out0;             // the query's 2 x n_peers words in the call's output
};
struct VerRes { int32_t status; int32_t order; uint32_t n; uint32_t pad; };   // n: words of a vector / ids of a frontiers (2 words each: peer index, counter)

struct VerCtx {
  const Dev* d; const DevDag* g; const DocMeta* m;
  uint32_t P; uint64_t vvh0;
  const uint32_t* end;       // [praw0 + p] the applied end of every peer
};

// peer index and node of the id, NONE where the applied history does not hold it
LM_DEV uint32_t ver_resolve(const VerCtx& x, const VerId& r, uint32_t& node) {
  const Dev& d = *x.d; const DocMeta& m = *x.m;
  node = NONE;
  if (r.neg || r.ctr >= MAX_COUNTER) return NONE;
  uint32_t lo = 0, hi = x.P;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (d.peer_uniq[m.praw0 + mid] < r.peer) lo = mid + 1; else hi = mid; }
  if (lo >= x.P || d.peer_uniq[m.praw0 + lo] != r.peer || r.ctr >= x.end[m.praw0 + lo]) return NONE;
  const uint32_t ci = find_change(d, m, lo, r.ctr);
  if (ci == NONE) return NONE;
  node = x.g->chg_node[m.chg0 + ci];
  return lo;
}

// One side: s_vv := the closure vector of the ids, s_cand[p] := the greatest counter + 1 among the ids of peer p (0: none),
// s_node[p] := its node.  false: an id the applied history does not hold.  fold = false: the candidates only (the heads need no vector)
LM_DEV bool ver_side(const VerCtx& x, const VerId* rows, uint32_t n, uint32_t* s_vv, uint32_t* s_cand, uint32_t* s_node, bool fold = true) {
  const int lane = lmw::lane();
  const uint32_t P = x.P;
  lmw::block_sync();
  for (uint32_t p = (uint32_t)lane; p < P; p += 64) { s_vv[p] = 0; s_cand[p] = 0; s_node[p] = NONE; }
  lmw::block_sync();
  bool ok = true;
  for (uint32_t i0 = 0; i0 < n; i0 += 64) {
    const bool mine = i0 + (uint32_t)lane < n;
    uint32_t pidx = NONE, ctr = 0, node = NONE;
    if (mine) { const VerId r = rows[i0 + (uint32_t)lane]; pidx = ver_resolve(x, r, node); ctr = r.ctr; }
    if (lmw::any(mine && pidx == NONE)) ok = false;
    for (uint64_t vm = lmw::ballot(pidx != NONE); vm; vm &= vm - 1) {
      const int s = lmw::ffs64(vm);
      const uint32_t q = lmw::bcast(pidx, s), c = lmw::bcast(ctr, s), nd = lmw::bcast(node, s);
      const uint32_t* hv = x.d->vvh + x.vvh0 + (uint64_t)nd * P;
      if (!fold) {   // (q's own lane, as in the loop below: one writer per word)
        if ((uint32_t)lane == (q & 63u) && c + 1 > s_cand[q]) { s_cand[q] = c + 1; s_node[q] = nd; }
        continue;
      }
      for (uint32_t p = (uint32_t)lane; p < P; p += 64) {
        uint32_t v = hv[p];
        if (p == q) {
          if (c + 1 > v) v = c + 1;
          if (c + 1 > s_cand[p]) { s_cand[p] = c + 1; s_node[p] = nd; }
        }
        if (v > s_vv[p]) s_vv[p] = v;
      }
    }
  }
  lmw::block_sync();
  return ok;
}

// the candidates of a version vector: the last id of every peer
LM_DEV void ver_cand_of_vector(const VerCtx& x, const uint32_t* end, uint32_t* s_cand, uint32_t* s_node) {
  const int lane = lmw::lane();
  lmw::block_sync();
  for (uint32_t p = (uint32_t)lane; p < x.P; p += 64) {
    const uint32_t e = end[x.m->praw0 + p];
    const uint32_t ci = e ? find_change(*x.d, *x.m, p, e - 1) : NONE;
    s_cand[p] = ci == NONE ? 0u : e;
    s_node[p] = ci == NONE ? NONE : x.g->chg_node[x.m->chg0 + ci];
  }
  lmw::block_sync();
}

// s_drop[p] := 1 where another candidate's closure holds the candidate of p
LM_DEV void ver_heads(const VerCtx& x, const uint32_t* s_cand, const uint32_t* s_node, uint32_t* s_drop) {
  const int lane = lmw::lane();
  const uint32_t P = x.P;
  for (uint32_t p = (uint32_t)lane; p < P; p += 64) s_drop[p] = 0;
  lmw::block_sync();
  for (uint32_t q0 = 0; q0 < P; q0 += 64) {
    const uint32_t ql = q0 + (uint32_t)lane;
    for (uint64_t qm = lmw::ballot(ql < P && s_cand[ql] != 0); qm; qm &= qm - 1) {
      const uint32_t q = q0 + (uint32_t)lmw::ffs64(qm);
      const uint32_t* hv = x.d->vvh + x.vvh0 + (uint64_t)s_node[q] * P;
      // (p != q states the definition and saves a compare; it cannot change an answer: vvh[node(q)][q] is the node head's own-peer
      // entry, at most the node's first counter, never above the candidate's)
      for (uint32_t p = (uint32_t)lane; p < P; p += 64)
        if (p != q && s_cand[p] != 0 && hv[p] > s_cand[p] - 1) s_drop[p] = 1;
    }
  }
  lmw::block_sync();
}

// the surviving candidates as (peer index, counter) pairs, ascending peer; returns their number
LM_DEV uint32_t ver_emit(const VerCtx& x, const uint32_t* s_cand, const uint32_t* s_drop, uint32_t* o) {
  const int lane = lmw::lane();
  uint32_t n = 0;
  for (uint32_t p0 = 0; p0 < x.P; p0 += 64) {
    const uint32_t p = p0 + (uint32_t)lane;
    const bool keep = p < x.P && s_cand[p] != 0 && !s_drop[p];
    const uint64_t km = lmw::ballot(keep);
    if (keep) {
      const uint32_t at = n + (uint32_t)lmw::popc64(km & ((1ull << lane) - 1));
      o[2 * at] = p; o[2 * at + 1] = s_cand[p] - 1;
    }
    n += (uint32_t)lmw::popc64(km);
  }
  return n;
}

LM_KERNEL void k_version(Dev d, DevDag g, const VerQuery* qs, const VerId* rows, VerRes* res, uint32_t* out) {
  const uint32_t b = (uint32_t)lmw::bid();
  const int lane = lmw::lane();
  const VerQuery Q = qs[b];
  const DocMeta m = d.doc[Q.doc];
  VerRes R;
  R.status = ST_OK; R.order = 0; R.n = 0; R.pad = 0;
  if (status_fatal(m.status) || m.n_peers > MAX_PEERS) {
    R.status = status_fatal(m.status) ? m.status : ST_UNSUPPORTED;
    if (lane == 0) res[b] = R;
    return;
  }
  VerCtx x;
  x.d = &d; x.g = &g; x.m = &m; x.P = m.n_peers; x.vvh0 = ((uint64_t)m.vvh0_hi << 32) | m.vvh0_lo;
  x.end = (d.res_vis || d.front_off[Q.doc + 1] > d.front_off[Q.doc]) ? d.peer_end_all : d.peer_end;
  const uint32_t P = x.P;
  uint32_t* o = out + Q.out0;
  LM_SHARED(uint32_t, s_va, MAX_PEERS);
  LM_SHARED(uint32_t, s_vb, MAX_PEERS);
  LM_SHARED(uint32_t, s_cand, MAX_PEERS);
  LM_SHARED(uint32_t, s_node, MAX_PEERS);
  LM_SHARED(uint32_t, s_drop, MAX_PEERS);
  if (Q.op == VER_TO_VV) {
    if (!ver_side(x, rows + Q.a0, Q.na, s_va, s_cand, s_node)) R.status = ST_FRONTIERS_NOT_FOUND;
    else { for (uint32_t p = (uint32_t)lane; p < P; p += 64) o[p] = s_va[p]; R.n = P; }
  } else if (Q.op == VER_TO_FRONTIERS || Q.op == VER_MINIMIZE) {
    if (!ver_side(x, rows + Q.a0, Q.na, s_va, s_cand, s_node, false)) R.status = ST_FRONTIERS_NOT_FOUND;
    else { ver_heads(x, s_cand, s_node, s_drop); R.n = ver_emit(x, s_cand, s_drop, o); }
  } else if (Q.op == VER_CMP) {
    const bool oka = ver_side(x, rows + Q.a0, Q.na, s_va, s_cand, s_node);
    const bool okb = ver_side(x, rows + Q.b0, Q.nb, s_vb, s_cand, s_node);
    if (!oka || !okb) R.status = ST_FRONTIERS_NOT_FOUND;
    else {
      bool lt = false, gt = false;
      for (uint32_t p = (uint32_t)lane; p < P; p += 64) { lt |= s_va[p] < s_vb[p]; gt |= s_va[p] > s_vb[p]; }
      lt = lmw::any(lt); gt = lmw::any(gt);
      R.order = lt && gt ? VER_CONCURRENT : lt ? VER_LESS : gt ? VER_GREATER : VER_EQUAL;
    }
  } else if (Q.op == VER_CMP_DOC) {
    // cmp_with_frontiers, literally: equal as sets to the document's heads -> 0; else every id below the applied vector (a vector
    // test, no DAG lookup) -> 1; else -1.  (The host hands the ids over without duplicates.)
    ver_cand_of_vector(x, x.end, s_cand, s_node);
    ver_heads(x, s_cand, s_node, s_drop);
    uint32_t n_heads = 0;
    for (uint32_t p0 = 0; p0 < P; p0 += 64) { const uint32_t p = p0 + (uint32_t)lane; n_heads += (uint32_t)lmw::popc64(lmw::ballot(p < P && s_cand[p] != 0 && !s_drop[p])); }
    bool not_head = false, not_in = false;
    for (uint32_t i = (uint32_t)lane; i < Q.na; i += 64) {
      const VerId r = rows[Q.a0 + i];
      uint32_t lo = 0, hi = P;
      while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (d.peer_uniq[m.praw0 + mid] < r.peer) lo = mid + 1; else hi = mid; }
      const bool known = !r.neg && lo < P && d.peer_uniq[m.praw0 + lo] == r.peer;
      if (!known || r.ctr >= x.end[m.praw0 + lo]) not_in = true;
      if (!known || s_drop[lo] || s_cand[lo] != r.ctr + 1) not_head = true;
    }
    not_head = lmw::any(not_head); not_in = lmw::any(not_in);
    R.order = (!not_head && Q.na == n_heads) ? VER_EQUAL : !not_in ? VER_GREATER : VER_LESS;
  } else {   // VER_HEADS: which = 0 the applied history, 1 the version the run rendered
    ver_cand_of_vector(x, Q.b0 ? d.peer_end : x.end, s_cand, s_node);
    ver_heads(x, s_cand, s_node, s_drop);
    R.n = ver_emit(x, s_cand, s_drop, o);
  }
  if (lane == 0) res[b] = R;
}

}  // namespace lm
