// TEST INFRASTRUCTURE ONLY (see emul.cpp): the fast path pass in blocks
#include "lane_ops_emul.h"
#include "../../deciphon_amd/csrc/viterbi_body.h"
#include "block_walk.h"

extern "C" int emul_path_blocks(float const *pool, DcpProfileDev const *pf, DcpCodeRow const *codes, int L, float const *xt,
                                int B, int G, uint32_t *buf, long cap, float *score)
{
  switch (pf->Q * 100 + pf->W)
  {
#define SHAPE(Q, W) \
  case Q * 100 + W: return em_path_blocks<CostWave<Q, W>, CostWave<Q, W, true>>(pool, *pf, codes, L, xt, B, G, buf, cap, score);
    SHAPE(1, 1) SHAPE(2, 1) SHAPE(3, 1) SHAPE(4, 1) SHAPE(6, 1) SHAPE(8, 1) SHAPE(6, 2) SHAPE(4, 4)
    SHAPE(6, 4) SHAPE(8, 4) SHAPE(8, 8) // every class of dcp_launch_path_blocks (tests/test_emul_block_edges.py)
#undef SHAPE
  default: return -100;
  }
}
