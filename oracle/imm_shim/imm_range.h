/* imm_range.h -- TEST INFRASTRUCTURE ONLY (oracle/Makefile `ref`).
 *
 * Stands in for the imm library's range header, which the reference's
 * c-core/window.c uses (through sequence.h).  Written for this repository.
 * It asserts these facts about imm:
 *   a range is {start, stop} of int, built by imm_range(start, stop);
 *   imm_range_size() is stop - start as a signed int (window.c compares it
 *   with a last hit position of -1).
 */
#ifndef IMM_RANGE_H
#define IMM_RANGE_H

struct imm_range
{
  int start;
  int stop;
};

static inline struct imm_range imm_range(int start, int stop) { return (struct imm_range){start, stop}; }

static inline int imm_range_size(struct imm_range x) { return x.stop - x.start; }

#endif
