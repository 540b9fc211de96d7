// traceback.h -- the path of a window from its DP table, without a trellis.
//
// The fast path pass: the cost kernel (CostWave<.., STORE>) leaves the final value of
// every state of every row in HBM; this walk then goes from T at row L back to S at row 0
// and, at each state it visits, re-evaluates that state's candidates exactly as the
// reference forms them -- (x + transition) + emission, c-core/viterbi.c:224,526-536 -- in
// the reference's order (t = 5..1; BM,MM,IM,DM / II,MI / EC,CC ...).  The reference keeps
// the FIRST candidate that attains the minimum (strict-< updates), so the back-pointer is
// the first candidate equal to the stored value: the same step trellis_unzip would read
// from the trellis (c-core/trellis.c:51-113,147-167), at O(path) instead of O(K*L*5) work.
//
// Where the reference's choice depends on more than the final values -- an exact fp32 tie
// between MD and DD, between the candidates of B or T, or a D state tying the row minimum E
// (c-core/viterbi.c:538-586 resolves those by pass history) -- the walk gives up
// (DCP_TB_TIE) and the caller runs the literal path kernel for that window.
//
// One source for the GPU, the host and the wave emulator (tests/emul): the candidates of the visited state are
// spread over the 64 lanes of a wavefront in the reference's order -- lane j = (5 - t) * names + name -- so that one
// step costs two load round trips instead of a chain of them, and the first candidate equal to the stored value is
// the lowest set bit of a ballot.  What crosses lanes goes through a lane policy:
//   leader()  : true on the lane that writes buf and *st
//   ballot(f) : 64-bit mask of f(lane) over the 64 lanes
//   max_of(f) : the maximum of f(lane) over the 64 lanes
// DcpLanesHost below takes the lanes one after the other; the wavefront's own is DcpLanesWave (lane_ops_gpu.h).
#pragma once
#include "dcp_states.h"

enum { DCP_TB_OVERFLOW = -1, DCP_TB_TIE = -2, DCP_TB_BAD = -3 };

struct DcpTraceIn
{
  int K, Kp, L;
  float const *sp;    // [(L+1)][DCP_SP_STRIDE]: N,B,J,E,C of every row
  float const *cells; // [(L+1)][3][Kp]: M,I,D
  float const *rows;  // profile emission rows [1364][DCP_ROW_HDR + Kp]
  float const *trans; // [8][Kp]
  DcpCodeRow const *codes; // row l = codes of the t-mers ending at window position l
  float const *xt;    // 13 special transitions
  // blocks (dcp_types.h): the table holds rows row_base .. and the walk stops, to be resumed on the block
  // before, at the first state whose stage is <= lo (lo < 0: never)
  int row_base = 0, lo = -1;
};

// A window's side of a DcpTraceIn; the table (sp, cells, row_base) and lo come with a block: dcp_trace_bind.
DCP_HDI DcpTraceIn dcp_trace_in(float const *pool, DcpProfileDev const &pf, DcpCodeRow const *codes, float const *xt, int L)
{
  DcpTraceIn in;
  in.K = pf.K;
  in.Kp = pf.Kp;
  in.L = L;
  in.sp = in.cells = nullptr;
  in.rows = pool + pf.rows_off;
  in.trans = pool + pf.trans_off;
  in.codes = codes;
  in.xt = xt;
  return in;
}

// `table` holds block blk of the window (dcp_types.h)
DCP_HDI void dcp_trace_bind(DcpTraceIn &in, float const *table, DcpBlock const &blk)
{
  in.sp = table;
  in.cells = table + (size_t)blk.slots * DCP_SP_STRIDE;
  in.row_base = blk.row_base;
  in.lo = blk.lo;
}

struct DcpLanesHost
{
  DCP_HDI static bool leader() { return true; }
  template <class F> DCP_HDI static uint64_t ballot(F f)
  {
    uint64_t mask = 0;
    for (int lane = 0; lane < 64; ++lane) mask |= (uint64_t)(f(lane) ? 1 : 0) << lane;
    return mask;
  }
  template <class F> DCP_HDI static int max_of(F f)
  {
    int best = f(0);
    for (int lane = 1; lane < 64; ++lane)
    {
      int const v = f(lane);
      best = v > best ? v : best;
    }
    return best;
  }
};

// Writes the steps (state_id | seqsize << 16) from the END of buf backwards; returns their
// number, or a DCP_TB_* code -- or 0 when the walk stopped at in.lo with where it stands in *st
// (st != NULL: resume from *st unless it is fresh, i.e. zeroed -- no state id is 0).
template <class Lanes = DcpLanesHost>
DCP_HDI int dcp_traceback(DcpTraceIn const &in, uint32_t *buf, int64_t cap, DcpTraceState *st = nullptr)
{
  float const INF = __builtin_inff();
  int const K = in.K, Kp = in.Kp;
  size_t const stride = (size_t)Kp + DCP_ROW_HDR;
  int const base = in.row_base;
  auto SP = [&](int l, int i) { return in.sp[(size_t)(l - base) * DCP_SP_STRIDE + i]; }; // 0 N, 1 B, 2 J, 3 E, 4 C
  auto CELL = [&](int l, int s, int k) { return k < 0 ? INF : in.cells[((size_t)(l - base) * 3 + s) * (size_t)Kp + k]; };
  auto TR = [&](int id, int k) { return in.trans[(size_t)id * Kp + k]; };
  float const *xt = in.xt;

  int state = ST_T, stage = in.L;
  int64_t n = 0;
  if (st && st->state != 0) // resume where the block after this one stopped (uniform: every lane reads the same)
  {
    state = st->state;
    stage = st->stage;
    n = st->n;
  }
  while (state != ST_S || stage)
  {
    if (stage <= in.lo) // the rest of the path lies in the block before this one
    {
      if (Lanes::leader())
      {
        st->state = state;
        st->stage = stage;
        st->n = n;
      }
      return 0;
    }
    int size = 0, prev = -1;
    DcpCodeRow const cr = in.codes[stage];
    if (!is_core(state))
    {
      if (state == ST_T)
      {
        float const a = SP(stage, 3) + xt[DCP_ET], b = SP(stage, 4) + xt[DCP_CT];
        if (a == b) return a < INF ? DCP_TB_TIE : DCP_TB_BAD;
        prev = a < b ? ST_E : ST_C;
      }
      else if (state == ST_N || state == ST_J || state == ST_C)
      {
        int const self = state == ST_N ? 0 : state == ST_J ? 2 : 4;
        float const target = SP(stage, self);
        if (!(target < INF)) return DCP_TB_BAD;
        float const t_in = state == ST_N ? xt[DCP_SN] : state == ST_J ? xt[DCP_EJ] : xt[DCP_EC];
        float const t_self = state == ST_N ? xt[DCP_NN] : state == ST_J ? xt[DCP_JJ] : xt[DCP_CC];
        uint64_t const mask = Lanes::ballot([&](int lane) {
          int const t = 5 - (lane >> 1), which = lane & 1; // from S (N) or E (J, C), then the state itself
          if (lane >= 10 || t > stage) return false;
          int const z = stage - t;
          float const nil = in.rows[(size_t)cr.c[t - 1] * stride];
          float const from = state == ST_N ? (z == 0 ? 0.0f : INF) : SP(z, 3); // S of row z, or E of row z
          float const cand = which == 0 ? (from + t_in) + nil : (SP(z, self) + t_self) + nil;
          return cand == target;
        });
        if (!mask) return DCP_TB_BAD;
        int const j = __builtin_ctzll(mask);
        size = 5 - (j >> 1);
        prev = (j & 1) ? state : (state == ST_N ? ST_S : ST_E);
      }
      else if (state == ST_B)
      {
        if (stage == 0) prev = ST_S; // row 0: B = S + SB (c-core/viterbi.c:473)
        else
        {
          float const target = SP(stage, 1);
          int const eN = SP(stage, 0) + xt[DCP_NB] == target, eE = SP(stage, 3) + xt[DCP_EB] == target,
                    eJ = SP(stage, 2) + xt[DCP_JB] == target;
          if (eN + eE + eJ != 1 || !(target < INF)) return eN + eE + eJ > 1 ? DCP_TB_TIE : DCP_TB_BAD;
          prev = eN ? ST_N : eE ? ST_E : ST_J;
        }
      }
      else if (state == ST_E)
      {
        // E = min over k of M (c-core/viterbi.c:540-558).  Several M equal to it: the
        // reference's lanes (k = e*Qr + q) keep the first q per lane and the highest lane.
        float const target = SP(stage, 3);
        if (!(target < INF)) return DCP_TB_BAD;
        int Qr = (K - 1) / DCP_REF_LANES + 1;
        if (Qr < 2) Qr = 2;
        // key = (reference lane << 16) | (65535 - k): highest lane, then lowest k; above every key, D_TIE
        int const D_TIE = 0x7fffffff;
        int const key = Lanes::max_of([&](int lane) {
          int best = -1;
          for (int k = lane; k < K; k += 64)
          {
            int const cand = CELL(stage, 2, k) == target   ? D_TIE // a D candidate at the minimum: pass history decides
                             : CELL(stage, 0, k) == target ? ((k / Qr) << 16) | (65535 - k)
                                                           : -1;
            best = cand > best ? cand : best;
          }
          return best;
        });
        if (key == D_TIE) return DCP_TB_TIE;
        if (key < 0) return DCP_TB_BAD;
        prev = ST_M | ((65535 - (key & 0xffff)) + 1);
      }
      else
        return DCP_TB_BAD;
    }
    else
    {
      int const k = core_idx(state);
      if (k < 0 || k >= K) return DCP_TB_BAD;
      if (msb(state) == ST_M)
      {
        float const target = CELL(stage, 0, k);
        if (!(target < INF)) return DCP_TB_BAD;
        uint64_t const mask = Lanes::ballot([&](int lane) {
          int const t = 5 - (lane >> 2), name = lane & 3; // BM, MM, IM, DM
          if (lane >= 20 || t > stage) return false;
          int const z = stage - t;
          float const m = in.rows[(size_t)cr.c[t - 1] * stride + DCP_ROW_HDR + k];
          float const x = name == 0 ? SP(z, 1) : CELL(z, name - 1, k - 1);
          float const tr = TR(name == 0 ? DCP_BM : name == 1 ? DCP_MM : name == 2 ? DCP_IM : DCP_DM, k);
          return (x + tr) + m == target;
        });
        if (!mask) return DCP_TB_BAD;
        int const j = __builtin_ctzll(mask);
        size = 5 - (j >> 2);
        int const nm = j & 3;
        prev = nm == 0 ? ST_B : (nm == 1 ? ST_M : nm == 2 ? ST_I : ST_D) | k;
      }
      else if (msb(state) == ST_I)
      {
        float const target = CELL(stage, 1, k);
        if (!(target < INF)) return DCP_TB_BAD;
        uint64_t const mask = Lanes::ballot([&](int lane) {
          int const t = 5 - (lane >> 1), name = lane & 1; // II, MI
          if (lane >= 10 || t > stage) return false;
          int const z = stage - t;
          float const bg = in.rows[(size_t)cr.c[t - 1] * stride + 1];
          float const x = name == 0 ? CELL(z, 1, k) : CELL(z, 0, k);
          float const tr = TR(name == 0 ? DCP_II : DCP_MI, k);
          return (x + tr) + bg == target;
        });
        if (!mask) return DCP_TB_BAD;
        int const j = __builtin_ctzll(mask);
        size = 5 - (j >> 1);
        prev = ((j & 1) ? ST_M : ST_I) | (k + 1);
      }
      else
      {
        float const a = CELL(stage, 0, k - 1) + TR(DCP_MD, k), b = CELL(stage, 2, k - 1) + TR(DCP_DD, k);
        if (a == b) return a < INF ? DCP_TB_TIE : DCP_TB_BAD;
        prev = (a < b ? ST_M : ST_D) | k;
      }
    }
    if (n + 1 >= cap) return DCP_TB_OVERFLOW;
    if (Lanes::leader()) buf[cap - 1 - n] = (uint32_t)state | ((uint32_t)size << 16);
    ++n;
    state = prev;
    stage -= size;
    if (stage < 0) return DCP_TB_BAD;
  }
  if (n >= cap) return DCP_TB_OVERFLOW;
  if (Lanes::leader()) buf[cap - 1 - n] = (uint32_t)state;
  return (int)(n + 1);
}

// Launch `it` of the groups of G blocks (dcp_types.h): the walk through the blocks that the launch left in the window's
// G tables (the first at `tables`), the highest first.  Returns what dcp_traceback does: 0 when the walk stands at the
// lower end of the last of them, or the window had no block in this launch.
template <class Lanes = DcpLanesHost>
DCP_HDI int dcp_traceback_group(DcpTraceIn &in, float const *tables, int B, int G, int it, uint32_t *buf, int64_t cap,
                                DcpTraceState *st)
{
  int r = 0;
  for (int sub = 0; sub < G && r == 0; ++sub)
  {
    int const j = dcp_group_block(in.L, B, G, it, sub);
    if (j < 0) break;
    dcp_trace_bind(in, tables + dcp_group_table(in.L, in.Kp, B, sub), dcp_block(in.L, B, j));
    r = dcp_traceback<Lanes>(in, buf, cap, st);
  }
  return r;
}
