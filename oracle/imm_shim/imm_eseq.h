/* imm_eseq.h -- TEST INFRASTRUCTURE ONLY (oracle/Makefile `ref`).
 *
 * Stands in for the imm library's sequence headers, which the reference's
 * c-core/sequence.h includes, so that window.c compiles.  Placeholders only:
 * window.c reaches a sequence through sequence_size() and sequence_slice(),
 * which oracle/ref_glue.c restates over a plain length kept in imm_seq.size.
 * Asserts no fact about imm beyond the type names.
 */
#ifndef IMM_ESEQ_H
#define IMM_ESEQ_H

struct imm_code;

struct imm_seq
{
  int size;
};

struct imm_eseq
{
  int unused;
};

#endif
