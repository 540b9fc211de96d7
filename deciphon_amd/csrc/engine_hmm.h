// engine_hmm.h -- the C++ entry behind dcp_hip_load_hmm (engine_profiles.cpp), for the scan: the same load, and every
// profile that is loaded is shown to a sink while its model is at hand.  Inside the library only (exports.map).
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
