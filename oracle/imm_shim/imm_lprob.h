/* imm_lprob.h -- TEST INFRASTRUCTURE ONLY (oracle/Makefile `ref`).
 *
 * Stands in for the imm library's log-probability header, which the
 * reference's c-core/xtrans.c includes.  Written for this repository; it
 * asserts two facts about imm and nothing else:
 *   IMM_LPROB_ONE  is log(1) =  0 (float),
 *   IMM_LPROB_ZERO is log(0) = -inf (float).
 * The real header brings <math.h> with it (it needs INFINITY); so does this
 * one, and xtrans.c's log() / logf() are those of <math.h>.
 */
#ifndef IMM_LPROB_H
#define IMM_LPROB_H

#include <math.h>

#define IMM_LPROB_ONE 0.0f
#define IMM_LPROB_ZERO (-INFINITY)

#endif
