// path_plan.cpp -- the memory plan of the path pass (path_plan.h).
#include "path_plan.h"

#include <algorithm>

namespace
{

size_t aligned256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// the replay scratch of the literal pass: three rows of K floats per row of the trellis served (row_replay.h)
size_t scratch_bytes(int rows, int K) { return (size_t)rows * 3 * (size_t)K * sizeof(float); }

// one block's table, then the window's checkpoints (16-byte aligned)
size_t block_table_bytes(int L, int Kp, int B) { return (size_t)dcp_block_slots(L, B) * (DCP_SP_STRIDE + 3 * (size_t)Kp) * 4; }
// (strip: a window of the strip class, whose checkpoints carry B of five rows as well)
size_t ckpt_bytes(int L, int Kp, int W, int B, bool strip)
{
  return (size_t)(dcp_num_blocks(L, B) - 1) * (size_t)(strip ? dcp_strip_ckpt_floats(Kp, W) : dcp_ckpt_floats(Kp, W)) * 4;
}
// the G tables of a window whose G blocks are computed at once (dcp_cost_store_kernel); its checkpoints come behind them
size_t group_tables_bytes(int L, int Kp, int B, int G)
{
  return ((size_t)std::min(G, dcp_num_blocks(L, B)) * block_table_bytes(L, Kp, B) + 15) & ~(size_t)15;
}

// Does this window of the strip class go in blocks?  `whole` = what it takes otherwise: its whole table (fast pass),
// or that and the replay scratch of all its rows (literal pass).  Where that fits the budget the window keeps it: its
// rows are walked once instead of twice.  Where it does not the window is taken a block at a time like every other
// class -- unless the budget is strict: DECIPHON_HIP_PATH_STRICT=1 refuses a strip window whose WHOLE table exceeds the
// budget, as it always has (its block table might fit; the rule is kept because callers and tests rely on it).
bool strip_in_blocks(size_t whole, int B, size_t budget, bool strict) { return B > 0 && whole > budget && !strict; }

// The G block tables, the checkpoints and (literal pass) the replay scratch of a window are ONE placement, and a
// placement lies in one chunk of the arena.  Once the arena holds chunks -- dcp_hip_path_reserve sets the whole budget
// aside in chunks of TableArena::CHUNK -- a placement beyond the largest of them would be allocated on top of what is
// held, outside the budget: G is held to what a chunk takes.  per_block, fixed: bytes of one more block, of the rest.
int group_chunk_cap(size_t chunk, size_t per_block, size_t fixed)
{
  if (chunk == 0 || per_block == 0) return INT32_MAX; // nothing held yet: the first chunk is made to measure
  size_t const slack = 1024; // the alignments of group_tables_bytes and TableArena::place
  return chunk > fixed + slack + per_block ? (int)std::min<size_t>((chunk - fixed - slack) / per_block, (size_t)INT32_MAX) : 1;
}

// How many blocks of a window go side by side: what 90 % of the budget holds of them at `one` bytes each beside
// `fixed`, no more than the window with the most blocks has (`most`) or a chunk takes (`cap`, group_chunk_cap).
// forced > 0 (DECIPHON_HIP_PATH_GROUP) replaces all that but `most`.
int group_size(size_t budget, double fixed, double one, int most, int cap, int forced)
{
  double const room = 0.9 * (double)budget - fixed;
  int G = one > 0 && room > one ? (int)std::min<double>(room / one, (double)most) : 1;
  G = std::min(G, cap);
  if (forced > 0) G = forced;
  return std::max(1, std::min(G, most));
}

} // namespace

DcpPathPlan dcp_plan_path(DcpPathKind kind, int n, DcpPathWindow const *w, int B, size_t budget, bool strict,
                          size_t largest_chunk, int group_override)
{
  bool const literal = kind == DCP_PATH_LITERAL;
  DcpPathPlan plan;
  plan.B = B;
  plan.place.assign((size_t)std::max(n, 0), DcpPathPlace{true, 1, 0, 0, 0, 0});
  // Fast pass: as many blocks side by side as the budget holds tables for, for ALL the windows of the request at once
  // -- with few hits every block of every window (the rows of a window are then walked once by one wavefront, for the
  // checkpoints, and once by many); with many hits one (a slice of windows fills the GPU by itself).  Literal pass: as
  // many as the budget holds for the window that needs the most.
  double fixed = 0, one = 0;
  int most = 1, cap = INT32_MAX;
  for (int i = 0; i < n; ++i)
  {
    DcpPathWindow const &v = w[i];
    DcpPathPlace &p = plan.place[(size_t)i];
    bool const strip = literal || v.strip;
    size_t const table = dcp_table_bytes(v.L, v.Kp);
    p.in_blocks = !strip || strip_in_blocks(literal ? aligned256(table) + scratch_bytes(v.L + 1, v.K) : table, B, budget, strict);
    if (!p.in_blocks)
    {
      if (!literal) fixed += (double)table;
      continue;
    }
    p.blocks = dcp_num_blocks(v.L, B);
    plan.blocked += strip;
    size_t const per_block = block_table_bytes(v.L, v.Kp, B) + (literal ? scratch_bytes(dcp_replay_block_rows(B), v.K) : 0);
    size_t const ckpts = ckpt_bytes(v.L, v.Kp, v.W, B, strip);
    one = literal ? std::max(one, (double)per_block) : one + (double)per_block;
    fixed = literal ? std::max(fixed, (double)ckpts) : fixed + (double)ckpts;
    most = std::max(most, p.blocks);
    cap = std::min(cap, group_chunk_cap(largest_chunk, per_block, ckpts));
  }
  int const G = plan.G = group_size(budget, fixed, one, most, cap, group_override);
  // one placement per window: its table(s), then the checkpoints, then (literal pass) the scratch
  for (int i = 0; i < n; ++i)
  {
    DcpPathWindow const &v = w[i];
    DcpPathPlace &p = plan.place[(size_t)i];
    p.ckpt_off = p.in_blocks ? group_tables_bytes(v.L, v.Kp, B, G) : 0;
    p.bytes = p.in_blocks ? p.ckpt_off + ckpt_bytes(v.L, v.Kp, v.W, B, literal || v.strip) : dcp_table_bytes(v.L, v.Kp);
    if (!literal) continue;
    p.replay_rows = p.in_blocks ? std::min(G, p.blocks) * dcp_replay_block_rows(B) : v.L + 1;
    p.scratch_off = aligned256(p.bytes);
    p.bytes = p.scratch_off + scratch_bytes(p.replay_rows, v.K);
  }
  return plan;
}
