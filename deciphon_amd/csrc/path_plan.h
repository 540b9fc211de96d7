// path_plan.h -- the memory plan of the path pass: which windows are taken a block at a time, how many blocks go side by
// side, what a window places in the table arena and where its checkpoints and replay scratch lie in that placement.
// Host only: no GPU, no engine, no environment -- engine_path.cpp reads DECIPHON_HIP_CKPT_ROWS, _PATH_BUDGET_MB,
// _PATH_STRICT and _PATH_GROUP and passes the values in.  The block geometry itself is dcp_types.h's.
#pragma once
#include "dcp_types.h"
#include <stddef.h>
#include <vector>

// DP table of one window: float specials[(L+1)][8], float cells[(L+1)][3][Kp] (traceback.h)
inline size_t dcp_table_bytes(int L, int Kp) { return ((size_t)L + 1) * (DCP_SP_STRIDE + 3 * (size_t)Kp) * 4; }

// one window of the request, in the order planned: rows, positions, padded positions, wavefronts, strip class (K > 4096)
struct DcpPathWindow
{
  int L, K, Kp, W;
  bool strip;
};

// What one window places, as ONE placement (a placement lies in one chunk of the arena): the tables of min(G, blocks)
// blocks, or the whole table; behind them the checkpoints; behind those, from a multiple of 256, the replay scratch.
struct DcpPathPlace
{
  bool in_blocks;     // strip class: the table is held a block at a time; other classes: always true
  int blocks;         // dcp_num_blocks(L, B) when in_blocks, else 1
  int replay_rows;    // literal plan only: rows of scratch, min(G, blocks) * dcp_replay_block_rows(B), or L + 1
  size_t ckpt_off;    // bytes from the placement's start to the checkpoints; 0 = none (whole table)
  size_t scratch_off; // literal plan only: bytes to the replay scratch, [replay_rows][3][K] floats
  size_t bytes;       // what is handed to TableArena::place
};

struct DcpPathPlan
{
  int B = 0;       // rows between checkpoints, as given
  int G = 1;       // blocks of a window computed side by side
  int blocked = 0; // strip windows in blocks
  std::vector<DcpPathPlace> place;
};

// DCP_PATH_FAST: every window of a request, G from the SUM over its windows (all of them hold their tables at once
// where the budget allows).  DCP_PATH_LITERAL: its strip windows only (`strip` is not read), each with the replay
// scratch of its rows, G from the window that needs the MOST.
enum DcpPathKind { DCP_PATH_FAST, DCP_PATH_LITERAL };

// budget: bytes the arena may hold; strict: a strip window whose whole table exceeds it keeps the whole table all the
// same (and is then refused by the arena); largest_chunk: TableArena::largest_chunk(), 0 = nothing held yet;
// group_override > 0: G, whatever the budget and the chunks say (still no more than the most blocks a window has).
DcpPathPlan dcp_plan_path(DcpPathKind kind, int n, DcpPathWindow const *w, int B, size_t budget, bool strict,
                          size_t largest_chunk, int group_override);
