// dcp_states.h -- the state ids of a path and the decoding of one trellis step, for host code, HIP kernels and
// the wave emulator alike.
#pragma once
#include <stddef.h>

#include "dcp_types.h"

enum
{
  ST_M = 0 << 14, ST_I = 1 << 14, ST_D = 2 << 14, ST_X = 3 << 14, // c-core/state.h:9-25
  ST_S = ST_X | 3, ST_N = ST_X | 4, ST_B = ST_X | 5, ST_E = ST_X | 6, ST_J = ST_X | 7, ST_C = ST_X | 8, ST_T = ST_X | 9,
};
DCP_HDI int msb(int id) { return id & ST_X; }
DCP_HDI bool is_core(int id) { return msb(id) != ST_X; }
DCP_HDI int core_idx(int id) { return (id & 0x3FFF) - 1; }

// One step of trellis_unzip (c-core/trellis.c:147-167): previous_state and emission_size (:51-113) of `state` at
// row `stage` of the trellis xnodes[L+1], nodes[(L+1)*K].  prev < 0: the trellis is inconsistent there.
struct DcpStep
{
  int prev, size;
};
DCP_HDI DcpStep dcp_trellis_step(int K, uint32_t const *xnodes, uint16_t const *nodes, int state, int stage)
{
  DcpStep const invalid = {-1, 0};
  int size = 0, prev = -1;
  // field offsets/widths: c-core/trellis.h:42-56, c-core/state.h:27-39
  if (!is_core(state))
  {
    uint32_t const x = xnodes[stage];
    if (state == ST_N) { unsigned v = x & 0xF; size = (int)(v % 5) + 1; prev = v / 5 ? ST_N : ST_S; }
    else if (state == ST_B) { unsigned v = (x >> 4) & 0x3; prev = v == 0 ? ST_S : v == 1 ? ST_N : v == 2 ? ST_E : ST_J; }
    else if (state == ST_E) { unsigned v = (x >> 6) & 0x7FFF; prev = (v & 1 ? ST_D : ST_M) | (int)(v / 2 + 1); }
    else if (state == ST_C) { unsigned v = (x >> 21) & 0xF; size = (int)(v % 5) + 1; prev = v / 5 ? ST_C : ST_E; }
    else if (state == ST_T) { unsigned v = (x >> 25) & 0x1; prev = v ? ST_C : ST_E; }
    else if (state == ST_J) { unsigned v = (x >> 26) & 0xF; size = (int)(v % 5) + 1; prev = v / 5 ? ST_J : ST_E; }
    else return invalid;
  }
  else
  {
    int const idx = core_idx(state);
    if (idx < 0 || idx >= K) return invalid;
    uint16_t const w = nodes[(size_t)stage * (size_t)K + (size_t)idx];
    if (msb(state) == ST_M)
    {
      unsigned v = w & 0x1F;
      size = (int)(v % 5) + 1;
      unsigned s = v / 5;
      if (s == 0) prev = ST_B;
      else if (idx <= 0) return invalid; // BUG_ON(idx <= 0), c-core/trellis.c:72
      else prev = (s == 1 ? ST_M : s == 2 ? ST_I : ST_D) | idx;
    }
    else if (msb(state) == ST_D)
    {
      unsigned v = (w >> 5) & 0x1;
      if (idx <= 0) return invalid;
      prev = (v ? ST_D : ST_M) | idx;
    }
    else
    {
      unsigned v = (w >> 6) & 0xF;
      size = (int)(v % 5) + 1;
      prev = (v / 5 ? ST_I : ST_M) | (idx + 1);
    }
  }
  return {prev, size};
}
