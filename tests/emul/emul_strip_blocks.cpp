// TEST INFRASTRUCTURE ONLY (see emul.cpp): the strip class (K > 4096, StripWave) a block at a time.
// A library of its own (strip_blocks.mk): the counters that lane_ops_emul.h declares are defined here.
#include "lane_ops_emul.h"
#include "../../deciphon_amd/csrc/viterbi_body.h"
#include "block_walk.h"

thread_local long em_votes = 0, em_votes_true = 0;
thread_local long em_fallback_rows = 0;
thread_local long em_row_range_zeros = 0;

// f<Q, W>() for the shapes of emul_strip.cpp
#define STRIP_SHAPES(pf, f, ...) \
  switch ((pf)->Q * 100 + (pf)->W) \
  { \
  case 101: return f<StripWave<1, 1>, StripWave<1, 1, true>>(__VA_ARGS__); \
  case 201: return f<StripWave<2, 1>, StripWave<2, 1, true>>(__VA_ARGS__); \
  case 102: return f<StripWave<1, 2>, StripWave<1, 2, true>>(__VA_ARGS__); \
  case 202: return f<StripWave<2, 2>, StripWave<2, 2, true>>(__VA_ARGS__); \
  case 402: return f<StripWave<4, 2>, StripWave<4, 2, true>>(__VA_ARGS__); \
  case 104: return f<StripWave<1, 4>, StripWave<1, 4, true>>(__VA_ARGS__); \
  default: return -100; \
  }

extern "C" int emul_strip_path_blocks(float const *pool, DcpProfileDev const *pf, DcpCodeRow const *codes, int L,
                                      float const *xt, int B, int G, uint32_t *buf, long cap, float *score)
{
  STRIP_SHAPES(pf, em_path_blocks, pool, *pf, codes, L, xt, B, G, buf, cap, score)
}

extern "C" int emul_strip_replay_blocks(float const *pool, DcpProfileDev const *pf, DcpCodeRow const *codes, int L,
                                        float const *xt, int B, int G, uint32_t *xnodes, uint16_t *nodes, float *score)
{
  STRIP_SHAPES(pf, em_replay_blocks, pool, *pf, codes, L, xt, B, G, xnodes, nodes, score)
}

// dwords of emission rows answered by the range rule of load_row_q since the last call (lane_ops_emul.h)
extern "C" long emul_row_range_zeros(void)
{
  long const n = em_row_range_zeros;
  em_row_range_zeros = 0;
  return n;
}
