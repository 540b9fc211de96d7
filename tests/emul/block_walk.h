// TEST INFRASTRUCTURE ONLY (see emul.cpp): the path pass in blocks as the engine walks it, for CostWave and StripWave.
// The geometry is not restated here: blocks, tables and checkpoints come from dcp_block and its neighbours
// (dcp_types.h), the waves and the walks are bound to them by the binders the kernels use, and the walk through a
// launch's tables and the replay's threads are dcp_traceback_group and dcp_replay_thread themselves.
#pragma once
#include "../../deciphon_amd/csrc/row_replay.h"
#include <algorithm>
#include <new>
#include <vector>

template <class Wave> auto em_set_ring(Wave &w, float *ring, int) -> decltype((void)(w.ring = ring)) { w.ring = ring; }
template <class Wave> void em_set_ring(Wave &, float *, long) {} // CostWave keeps its ring in registers

// a wave as a kernel declares it, with nothing left from the call before (in place: too large for the stack)
template <class Wave> Wave &em_fresh_wave()
{
  static thread_local Wave w;
  return *new (&w) Wave();
}

// The checkpoints of a window (Ckpt), then launches it = 0, 1, .. of G blocks side by side (Store) into G tables
// dcp_block_table_floats apart: after(it, tables) after each, until it returns non-zero.  The checkpoints hold NaN
// until they are written, all G tables before every launch and the ring before every block: nothing may be read that
// was not written for it.
template <class Ckpt, class Store, class F>
int em_walk_blocks(float const *pool, DcpProfileDev const &pf, DcpCodeRow const *codes, int L, float const *xt, int B,
                   int G, float *score, F after)
{
  if (B < 0 || B % 5 || G < 1) return -100;
  int const nb = dcp_num_blocks(L, B);
  std::vector<float> ckpt((size_t)(nb - 1) * (size_t)Ckpt::ckpt_floats(pf.Kp), NAN), ring((size_t)10 * pf.Kp, NAN);
  std::vector<float> tables((size_t)G * (size_t)dcp_block_table_floats(L, pf.Kp, B));
  float out[2] = {NAN, NAN};
  if (nb > 1)
  {
    Ckpt &w = em_fresh_wave<Ckpt>();
    em_set_ring(w, ring.data(), 0);
    w.ckpt_out = ckpt.data();
    w.ckpt_every = B;
    w.init(pool, pf, codes, xt);
    w.run(L, out);
  }
  int r = 0;
  for (int it = 0; it * G < nb && r == 0; ++it)
  {
    std::fill(tables.begin(), tables.end(), NAN);
    for (int sub = 0; sub < G; ++sub)
    {
      int const j = dcp_group_block(L, B, G, it, sub);
      if (j < 0) break;
      DcpBlock const blk = dcp_block(L, B, j);
      std::fill(ring.begin(), ring.end(), NAN);
      Store &w = em_fresh_wave<Store>();
      em_set_ring(w, ring.data(), 0);
      dcp_bind_block(w, tables.data() + dcp_group_table(L, pf.Kp, B, sub), ckpt.data(), blk, pf.Kp);
      w.init(pool, pf, codes, xt);
      w.run(L, out, blk.last);
    }
    r = after(it, tables.data());
  }
  *score = out[1];
  return r;
}

// the fast path pass: the traceback resumed from launch to launch; returns what dcp_traceback does
template <class Ckpt, class Store>
int em_path_blocks(float const *pool, DcpProfileDev const &pf, DcpCodeRow const *codes, int L, float const *xt, int B, int G,
                   uint32_t *buf, long cap, float *score)
{
  DcpTraceState st;
  memset(&st, 0, sizeof st);
  DcpTraceIn in = dcp_trace_in(pool, pf, codes, xt, L);
  return em_walk_blocks<Ckpt, Store>(pool, pf, codes, L, xt, B, G, score, [&](int it, float const *tables) {
    return dcp_traceback_group(in, tables, B, G, it, buf, cap, &st);
  });
}

// the literal pass: the trellis replayed from the same tables, a launch's threads one after the other (whole
// wavefronts of them, as dcp_launch_replay starts)
template <class Ckpt, class Store>
int em_replay_blocks(float const *pool, DcpProfileDev const &pf, DcpCodeRow const *codes, int L, float const *xt, int B,
                     int G, uint32_t *xnodes, uint16_t *nodes, float *score)
{
  DcpTraceIn in = dcp_trace_in(pool, pf, codes, xt, L);
  int const rows = G * dcp_block_slots(L, B);
  std::vector<float> scratch((size_t)rows * 3 * pf.K, NAN);
  return em_walk_blocks<Ckpt, Store>(pool, pf, codes, L, xt, B, G, score, [&](int it, float const *tables) {
    for (int r = 0; r < (rows + 63) / 64 * 64; ++r) dcp_replay_thread(in, tables, B, G, it, r, scratch.data(), xnodes, nodes);
    return 0;
  });
}
