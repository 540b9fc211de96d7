// engine_hmm.h -- the C++ entries behind dcp_hip_load_hmm and dcp_hip_set_gencode (engine_hmm.cpp), for the scan: the
// same calls, and what is loaded or recomputed is shown to a sink while it is at hand.  Inside the library only
// (exports.map).
#pragma once
#include "../../include/deciphon_hip.h"
#include "hmm_model.h"

struct DcpHmmSink
{
  virtual ~DcpHmmSink() = default;
  // once, before the first profile: the null model and the background, the same for every profile of the file
  virtual void models(DcpNucltDist const &null, DcpNucltDist const &bg) = 0;
  // each profile of [first, first + count), in order.  When the load fails afterwards the engine keeps none of them:
  // the sink's owner drops what it was shown.
  virtual void profile(DcpHmmProfile const &p) = 0;
};

// dcp_hip_load_hmm (include/deciphon_hip.h); sink may be nullptr
int dcp_hip_load_hmm_sink(struct dcp_hip *, char const *hmm, int gencode_id, float epsilon, int first, int count,
                          DcpHmmSink *sink);

// What dcp_hip_set_gencode recomputes, shown while it is at hand: the scan's distributions come from the same call of
// dcp_setup_nuclt_dist as the engine's.
struct DcpGencodeSink
{
  virtual ~DcpGencodeSink() = default;
  // once, before the first entry, when nothing can be refused any more: the table, its null model and its background
  virtual void regencoded(int gencode_id, DcpNucltDist const &null, DcpNucltDist const &bg) = 0;
  // kept entries [first, first + n) -- the nodes of the profiles in engine order -- as they go up (press_kernel.h:
  // DCP_PRESS_IN_STRIDE floats each); ascending, every entry once
  virtual void entries(size_t first, size_t n, float const *in) = 0;
};

// dcp_hip_set_gencode (include/deciphon_hip.h); sink may be nullptr
int dcp_hip_set_gencode_sink(struct dcp_hip *, int gencode_id, DcpGencodeSink *sink);
