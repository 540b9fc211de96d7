// TEST INFRASTRUCTURE ONLY (see emul.cpp): the strip class (K > 4096, StripWave) a block at a time.
// A library of its own (strip_blocks.mk): the counters that lane_ops_emul.h declares are defined here.
#include "lane_ops_emul.h"
#include "../../deciphon_amd/csrc/viterbi_body.h"
#include "../../deciphon_amd/csrc/traceback.h"
#include "../../deciphon_amd/csrc/row_replay.h"
#include <vector>

thread_local long em_votes = 0, em_votes_true = 0;
thread_local long em_fallback_rows = 0;

namespace
{

// the checkpoints of a window, then its blocks from the last to the first: f(block, table) after each, until it
// returns non-zero.  The table (dcp_block_slots rows) and the ring hold NaN before every block: nothing may be read
// that this block did not write.
template <int Q, int W, class F>
int strip_blocks_qw(float const *pool, DcpProfileDev const &pf, DcpCodeRow const *codes, int L, float const *xt, int B,
                    float *score, F f)
{
  int const nb = dcp_num_blocks(L, B);
  size_t const cf = (size_t)dcp_strip_ckpt_floats(pf.Kp, W);
  std::vector<float> ckpt((size_t)(nb - 1) * cf, NAN), ring((size_t)10 * pf.Kp, NAN);
  float out[2] = {NAN, NAN};
  if (nb > 1)
  {
    static thread_local StripWave<Q, W> w;
    w = StripWave<Q, W>();
    w.ring = ring.data();
    w.ckpt_out = ckpt.data();
    w.ckpt_every = B;
    w.init(pool, pf, codes, xt);
    w.run(L, out);
  }
  int const slots = dcp_block_slots(L, B);
  std::vector<float> sp((size_t)slots * DCP_SP_STRIDE), cells((size_t)slots * 3 * pf.Kp);
  int r = 0;
  for (int block = nb - 1; block >= 0 && r == 0; --block)
  {
    std::fill(sp.begin(), sp.end(), NAN);
    std::fill(cells.begin(), cells.end(), NAN);
    std::fill(ring.begin(), ring.end(), NAN);
    static thread_local StripWave<Q, W, true> w;
    w = StripWave<Q, W, true>();
    w.ring = ring.data();
    w.tab_sp = sp.data();
    w.tab_cells = cells.data();
    w.row_base = block * B;
    w.ckpt_in = block > 0 ? ckpt.data() + (size_t)(block - 1) * cf : nullptr;
    w.init(pool, pf, codes, xt);
    int const last = B > 0 ? (block + 1) * B + 5 : L;
    w.run(L, out, last < L ? last : L);
    DcpTraceIn in = dcp_trace_in(pool, pf, codes, xt, L);
    in.sp = sp.data();
    in.cells = cells.data();
    in.row_base = block * B;
    in.lo = block > 0 ? block * B + 5 : -1;
    r = f(block, in);
  }
  *score = out[1];
  return r;
}

template <class F>
int strip_blocks(float const *pool, DcpProfileDev const &pf, DcpCodeRow const *codes, int L, float const *xt, int B,
                 float *score, F f)
{
  if (B < 0 || B % 5) return -100;
  switch (pf.Q * 100 + pf.W) // the shapes of emul_strip.cpp
  {
  case 101: return strip_blocks_qw<1, 1>(pool, pf, codes, L, xt, B, score, f);
  case 201: return strip_blocks_qw<2, 1>(pool, pf, codes, L, xt, B, score, f);
  case 102: return strip_blocks_qw<1, 2>(pool, pf, codes, L, xt, B, score, f);
  case 202: return strip_blocks_qw<2, 2>(pool, pf, codes, L, xt, B, score, f);
  case 402: return strip_blocks_qw<4, 2>(pool, pf, codes, L, xt, B, score, f);
  case 104: return strip_blocks_qw<1, 4>(pool, pf, codes, L, xt, B, score, f);
  default: return -100;
  }
}

} // namespace

// the fast path pass: the traceback resumed from block to block; returns what dcp_traceback does
extern "C" int emul_strip_path_blocks(float const *pool, DcpProfileDev const *pf, DcpCodeRow const *codes, int L,
                                      float const *xt, int B, uint32_t *buf, long cap, float *score)
{
  DcpTraceState st;
  memset(&st, 0, sizeof st);
  return strip_blocks(pool, *pf, codes, L, xt, B, score,
                      [&](int, DcpTraceIn const &in) { return dcp_traceback(in, buf, cap, &st); });
}

// the literal pass: the trellis replayed from the same blocks (row_replay.h), block j serving the rows of the
// traceback's partition, (j * B + 5, (j + 1) * B + 5] (block 0: from row 1)
extern "C" int emul_strip_replay_blocks(float const *pool, DcpProfileDev const *pf, DcpCodeRow const *codes, int L,
                                        float const *xt, int B, uint32_t *xnodes, uint16_t *nodes, float *score)
{
  int const K = pf->K;
  std::vector<float> acc((size_t)3 * K);
  xnodes[0] = 0;
  for (int k = 0; k < K; ++k) nodes[k] = 0;
  return strip_blocks(pool, *pf, codes, L, xt, B, score, [&](int block, DcpTraceIn const &in) {
    int const first = block > 0 ? block * B + 6 : 1, last = B > 0 && (block + 1) * B + 5 < L ? (block + 1) * B + 5 : L;
    for (int l = first; l <= last; ++l) dcp_replay_row(in, l, acc.data(), xnodes + l, nodes + (size_t)l * K);
    return 0;
  });
}
