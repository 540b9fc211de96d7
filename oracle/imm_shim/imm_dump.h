/* imm_dump.h -- TEST INFRASTRUCTURE ONLY (oracle/Makefile `ref`).
 *
 * Stands in for the imm library's dump header, which the reference's
 * c-core/xtrans.c includes for xtrans_dump().  Only the declaration: nothing
 * the tests run calls it, and oracle/ref_glue.c defines it so that the
 * library links.  Asserts no fact about imm beyond the signature.
 */
#ifndef IMM_DUMP_H
#define IMM_DUMP_H

#include <stddef.h>
#include <stdio.h>

void imm_dump_array_f32(size_t size, float const *array, FILE *restrict fp);

#endif
