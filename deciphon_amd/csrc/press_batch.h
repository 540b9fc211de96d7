// press_batch.h -- what dcp_press_* (press.cpp) and dcp_hip_load_hmm (engine_hmm.cpp) share: profiles read from a
// HMMER3 file into batches of whole profiles, and a batch's nodes laid out as the emission kernel's input.
#pragma once
#include "hmm_model.h"
#include "press_kernel.h"

#include <stdint.h>
#include <vector>

#define DCP_PRESS_BATCH_NODES 16384 // per launch (DECIPHON_HIP_PRESS_BATCH_NODES); a longer profile goes alone

// DECIPHON_HIP_PRESS_BATCH_NODES, or the default
int64_t dcp_press_batch_nodes();

// one input entry of the emission kernel (press_kernel.h): nucltp[4], codonm[125], 3 of padding
void dcp_press_put_entry(float *in, DcpNucltDist const &d);

// The profiles of one launch: node n of profile i is entry first[i] + n.
struct DcpPressBatch
{
  std::vector<DcpHmmProfile> profiles;
  std::vector<int64_t> first; // entry of each profile's node 0
  int64_t entries = 0;
  int rc_after = 0;       // the reader's error on the profile after these
  bool eof_after = false; // the file ends after these
  // every node's entry into in[entries][DCP_PRESS_IN_STRIDE]
  void put_entries(float *in) const;
};

// Takes profiles from a reader into batches of at most batch_nodes nodes, whole profiles only; the profile that did not
// fit the batch it was read for opens the next one.
struct DcpPressFeeder
{
  int64_t batch_nodes = DCP_PRESS_BATCH_NODES;
  DcpHmmProfile pending; // parsed, did not fit the batch it was read for
  bool have_pending = false;
  // *skip profiles are read and dropped first (a reader's error among them ends the batch as any other does); at most
  // *limit profiles are taken (< 0: no limit), after which the batch ends as at the end of the file, with nothing
  // more read.  Both count down.
  void fill(DcpHmmReader &reader, DcpPressBatch &b, long *skip = nullptr, long *limit = nullptr);
};
