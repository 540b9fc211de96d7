// press_kernel.h -- launch of the emission-table kernel of press (press_kernel.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#define DCP_PRESS_IN_STRIDE 132 // floats per input entry: nucltp[4], codonm[125], 3 of padding
#define DCP_PRESS_TABLE 1364    // floats per output row: DCP_TABLE_SIZE quasi-codon codes

// out[i * 1364 + code] = log P(code) of entry i = 0..entries-1, from in[i * 132 ..] (log-probabilities), under error
// rate epsilon.  Both arrays are device memory of at least that many rows.  Returns 0, or -1 when the launch failed.
int dcp_press_emission_launch(float const *in, float *out, int entries, float epsilon, hipStream_t stream);
