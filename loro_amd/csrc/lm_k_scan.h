// Exclusive prefix sums over interleaved u32 counters (rows × ncomp) — table offsets of the decode stage.
#pragma once
#include "lm_wave.h"

namespace lm {

static constexpr int SCAN_TILE = 256;

// phase 1: per-tile exclusive scan; out[row] = exclusive-in-tile, tile_sum[tile] = tile total
LM_KERNEL void k_scan_tile(const uint32_t* in, uint32_t* out, uint32_t* tile_sum, uint32_t n, uint32_t ncomp) {
  LM_SHARED(uint32_t, s_w, 4);
  uint32_t tile = (uint32_t)lmw::bid();
  uint32_t row = tile * SCAN_TILE + (uint32_t)lmw::tid();
  int lane = lmw::lane(), w = lmw::wave_in_block();
  for (uint32_t c = 0; c < ncomp; c++) {
    uint32_t v = row < n ? in[(uint64_t)row * ncomp + c] : 0;
    uint32_t inc = lmw::scan_incl_add(v);
    if (lane == 63) s_w[w] = inc;
    lmw::block_sync();
    uint32_t base = 0;
    for (int k = 0; k < w; k++) base += s_w[k];
    if (row < n) out[(uint64_t)row * ncomp + c] = base + inc - v;
    if (lmw::tid() == SCAN_TILE - 1) tile_sum[(uint64_t)tile * ncomp + c] = base + inc;
    lmw::block_sync();
  }
}
// phase 2: one wave scans the tile sums in place (exclusive)
LM_KERNEL void k_scan_sums(uint32_t* tile_sum, uint32_t n_tiles, uint32_t ncomp, uint32_t* totals) {
  int lane = lmw::lane();
  for (uint32_t c = 0; c < ncomp; c++) {
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 64) {
      uint32_t t = t0 + (uint32_t)lane;
      uint32_t v = t < n_tiles ? tile_sum[(uint64_t)t * ncomp + c] : 0;
      uint32_t inc = lmw::scan_incl_add(v);
      if (t < n_tiles) tile_sum[(uint64_t)t * ncomp + c] = run + inc - v;
      run += lmw::bcast(inc, 63);
    }
    if (lane == 0) totals[c] = run;
  }
}
// phase 3: add tile bases; row n receives the totals
LM_KERNEL void k_scan_add(uint32_t* out, const uint32_t* tile_sum, const uint32_t* totals, uint32_t n, uint32_t ncomp) {
  uint32_t tile = (uint32_t)lmw::bid();
  uint32_t row = tile * SCAN_TILE + (uint32_t)lmw::tid();
  for (uint32_t c = 0; c < ncomp; c++) {
    if (row < n) out[(uint64_t)row * ncomp + c] += tile_sum[(uint64_t)tile * ncomp + c];
    if (row == n) out[(uint64_t)row * ncomp + c] = totals[c];
  }
}

// wave-primitive self test, two parts per round:
//  * the DPP scan and the ballot count against the bpermute formulation on pseudo-random lane values;
//  * every cross-lane primitive the kernels use against a PLAIN LOOP over the lanes' inputs, which each lane first stores in LDS —
//    scan_incl_add / scan_incl_max, shift_up / shift_up0 by 1 and 2 (the lanes below the distance included: shift_up keeps the
//    lane's own value there, shift_up0 gives 0, and the kernels rely on both), row_down<4/8/12>, reduce_add / reduce_max /
//    reduce_min, shfl64 with a different source per lane, first.  The inputs go round four shapes: full 32-bit words (above 2^31:
//    the DPP builtins take `int`), one value in every lane, zeros, and zeros mixed with words whose top bit is set.
// One workgroup = one wave (the launch in lm_pipeline.h), so block_sync() orders the LDS stores and loads of both builds.
LM_KERNEL void k_selftest(uint32_t* out, uint32_t rounds) {
  LM_SHARED(uint32_t, s_in, 64);
  LM_SHARED(uint64_t, s_in64, 64);
  int lane = lmw::lane();
  uint32_t bad = 0;
  uint32_t x = 0x9E3779B9u * (uint32_t)(lane + 1) + (uint32_t)lmw::bid();
  for (uint32_t r = 0; r < rounds; r++) {
    x ^= x << 13; x ^= x >> 17; x ^= x << 5;
    uint32_t v = (r & 1) ? (x & 0xffff) : (x % 65u);
    uint32_t a = lmw::scan_incl_add(v), b = lmw::scan_incl_add_shfl(v);
    bad += a != b ? 1u : 0u;
    uint64_t m = lmw::ballot((v & 1) != 0);
    uint32_t c = (uint32_t)lmw::popc64(m & ((2ull << lane) - 1));
    uint32_t dref = lmw::scan_incl_add_shfl(v & 1);
    bad += c != dref ? 1u : 0u;
    // whole-wave shifts on the DPP crossbar vs the LDS permute
    uint32_t s1 = lmw::shift_up(x, 1), s2 = lmw::shift_up(x, 2), r1 = lmw::shfl_up(x, 1), r2 = lmw::shfl_up(x, 2);
    bad += s1 != r1 ? 1u : 0u;
    bad += s2 != r2 ? 1u : 0u;

    // ---- against a plain loop over the inputs in LDS
    uint32_t w;
    switch (r & 3u) {
      case 0: w = x; break;
      case 1: w = 0x9E3779B9u * (r + 1u) + (uint32_t)lmw::bid(); break;    // the same value in every lane
      case 2: w = 0u; break;
      default: w = (x & 0x10u) ? (x | 0x80000000u) : 0u; break;
    }
    const uint64_t w64 = ((uint64_t)x << 32) | (uint64_t)(w ^ 0xA5A5A5A5u);
    const int src = (lane * 7 + (int)r) & 63;
    lmw::block_sync();
    s_in[lane] = w; s_in64[lane] = w64;
    lmw::block_sync();
    uint32_t e_add = 0, e_max = 0, e_rmax = 0, e_rmin = 0xffffffffu, e_radd = 0;
    for (int i = 0; i < 64; i++) {
      uint32_t t = s_in[i];
      if (i <= lane) { e_add += t; e_max = t > e_max ? t : e_max; }
      e_radd += t; e_rmax = t > e_rmax ? t : e_rmax; e_rmin = t < e_rmin ? t : e_rmin;
    }
    bad += lmw::scan_incl_add(w) != e_add ? 1u : 0u;
    bad += lmw::scan_incl_max(w) != e_max ? 1u : 0u;
    bad += lmw::reduce_add(w) != e_radd ? 1u : 0u;
    bad += lmw::reduce_max(w) != e_rmax ? 1u : 0u;
    bad += lmw::reduce_min(w) != e_rmin ? 1u : 0u;
    bad += lmw::shift_up(w, 1) != (lane >= 1 ? s_in[lane - 1] : w) ? 1u : 0u;
    bad += lmw::shift_up(w, 2) != (lane >= 2 ? s_in[lane - 2] : w) ? 1u : 0u;
    bad += lmw::shift_up0(w, 1) != (lane >= 1 ? s_in[lane - 1] : 0u) ? 1u : 0u;
    bad += lmw::shift_up0(w, 2) != (lane >= 2 ? s_in[lane - 2] : 0u) ? 1u : 0u;
    bad += lmw::row_down<4>(w) != ((lane & 15) + 4 > 15 ? 0u : s_in[lane + 4]) ? 1u : 0u;
    bad += lmw::row_down<8>(w) != ((lane & 15) + 8 > 15 ? 0u : s_in[lane + 8]) ? 1u : 0u;
    bad += lmw::row_down<12>(w) != ((lane & 15) + 12 > 15 ? 0u : s_in[lane + 12]) ? 1u : 0u;
    bad += lmw::shfl64(w64, src) != s_in64[src] ? 1u : 0u;
    bad += lmw::first(w) != s_in[0] ? 1u : 0u;
  }
  // (the total by a plain loop as well: a broken reduce_add must not hide what the rounds counted)
  lmw::block_sync();
  s_in[lane] = bad;
  lmw::block_sync();
  if (lane == 0) { uint32_t tot = 0; for (int i = 0; i < 64; i++) tot += s_in[i]; out[lmw::bid()] = tot; }
}

// kept[] := 0 in front of the integrate stage (lm_pipeline.h): 16 bytes per lane and store, grid-stride.  (Rounds 5-6 cleared loc[]
// itself with it, 32 times the bytes.)  hipMemsetAsync's fill
// kernel wrote those 2 GB per 5,000 configs[1] documents at ≈2 TB/s (profiles/r06_kernel_stats.md: __amd_rocclr_fillBufferAligned,
// ≈1 ms per launch of the pipeline); HBM takes stores faster than that.
LM_KERNEL void k_fill_words(uint32_t* p, uint64_t n4, uint32_t v, uint32_t n_threads) {
  struct alignas(16) U4 { uint32_t x, y, z, w; };
  U4* q = (U4*)p;
  const U4 w4 = {v, v, v, v};
  for (uint64_t i = (uint64_t)lmw::bid() * (uint64_t)lmw::bdim() + (uint64_t)lmw::tid(); i < n4; i += n_threads) q[i] = w4;
}
// LM_LOC_POISON (tests) in a resident context, whose kept entries outlive a run: loc[slot] := v wherever the slot's kept[] bit is clear
// when this runs (lm_pipeline.h)
LM_KERNEL void k_fill_unkept(uint32_t* loc, const uint32_t* kept, uint64_t n, uint32_t v, uint32_t n_threads) {
  for (uint64_t i = (uint64_t)lmw::bid() * (uint64_t)lmw::bdim() + (uint64_t)lmw::tid(); i < n; i += n_threads)
    if (!((kept[i >> 5] >> (i & 31)) & 1u)) loc[i] = v;
}

}  // namespace lm
