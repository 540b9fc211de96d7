// press_batch.cpp -- see press_batch.h
#include "press_batch.h"

#include <stdlib.h>
#include <string.h>
#include <utility>

int64_t dcp_press_batch_nodes()
{
  if (char const *b = getenv("DECIPHON_HIP_PRESS_BATCH_NODES")) return atol(b) > 0 ? atol(b) : 1;
  return DCP_PRESS_BATCH_NODES;
}

void dcp_press_put_entry(float *in, DcpNucltDist const &d)
{
  memcpy(in, d.nucltp, sizeof d.nucltp);
  memcpy(in + 4, d.codonm, sizeof d.codonm);
  in[129] = in[130] = in[131] = 0.0f;
}

void DcpPressBatch::put_entries(float *in) const
{
  for (size_t i = 0; i < profiles.size(); ++i)
  {
    DcpHmmProfile const &p = profiles[i];
    for (int n = 0; n < p.core_size; ++n)
      dcp_press_put_entry(in + (size_t)(first[i] + n) * DCP_PRESS_IN_STRIDE, p.nodes[(size_t)n]);
  }
}

void DcpPressFeeder::fill(DcpHmmReader &reader, DcpPressBatch &b, long *skip, long *limit)
{
  b.profiles.clear();
  b.first.clear();
  b.entries = 0;
  b.rc_after = 0;
  b.eof_after = false;
  for (;;)
  {
    DcpHmmProfile p;
    if (have_pending)
    {
      p = std::move(pending);
      have_pending = false;
    }
    else
    {
      if (limit && *limit == 0)
      {
        b.eof_after = true;
        break;
      }
      int const rc = reader.next(p);
      if (rc)
      {
        b.rc_after = rc;
        break;
      }
      if (reader.end())
      {
        b.eof_after = true;
        break;
      }
      if (skip && *skip > 0)
      {
        --*skip;
        continue;
      }
      if (limit && *limit > 0) --*limit;
    }
    if (!b.profiles.empty() && b.entries + p.core_size > batch_nodes)
    {
      pending = std::move(p);
      have_pending = true;
      break;
    }
    b.first.push_back(b.entries);
    b.entries += p.core_size;
    b.profiles.push_back(std::move(p));
  }
}
