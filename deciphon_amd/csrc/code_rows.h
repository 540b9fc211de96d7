// code_rows.h -- what a code row is, stated once for the host (dcp_code_rows_of, host_logic.cpp) and for the kernels
// that write the rows (code_rows.hip).
//
// Row r of a sequence y holds in word t - 1, t = 1..5, the code of the t-mer y[r-t..r-1] that ends in front of it
// (imm_eseq_get, third-party imm): off[t] + the t-mer as a base-4 number, its leftmost symbol the most
// significant digit, A,C,G,T = 0..3 -- and 0 where the t-mer would begin before the sequence, r < t.  Words 5..7 of a
// row (DcpCodeRow) are 0.
#pragma once
#include "dcp_types.h"

// off[t], t = 1..5: the codes of the t-mers lie behind those of all shorter ones, 4 + 16 + .. + 4^(t-1)
DCP_HDI uint32_t dcp_code_off(int t)
{
  uint32_t const off[5] = {0u, 4u, 20u, 84u, 340u};
  return off[t - 1];
}

// Words 0..4 of the row that has `have` symbols to its left; sym(t) is the symbol t places to its left, asked for
// t = 1 .. min(have, 5) only, each once.
template <class Sym> DCP_HDI void dcp_code_row_words(int64_t have, Sym sym, uint32_t c[5])
{
  uint32_t idx = 0;
  for (int t = 1; t <= 5; ++t)
  {
    // the t-mer is the (t-1)-mer extended to the left: the new symbol is the most significant digit
    bool const ok = have >= t;
    uint32_t const s = ok ? (uint32_t)sym(t) : 0u;
    idx += s << (2 * (t - 1));
    c[t - 1] = ok ? dcp_code_off(t) + idx : 0u;
  }
}
