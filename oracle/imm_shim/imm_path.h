/* imm_path.h -- TEST INFRASTRUCTURE ONLY (oracle/Makefile `ref`).
 *
 * Stands in for the imm library's path header, which the reference's
 * c-core/trellis.c includes for trellis_unzip().  Written for this
 * repository.  It asserts these facts about imm:
 *   a step is (state id, sequence size, score), built by imm_step();
 *   imm_path_add() appends one step and returns non-zero when it cannot;
 *   imm_path_reverse() reverses the steps in place.
 * The path here is a caller-owned buffer of fixed capacity (oracle/ref_glue.c
 * ref_unzip): a full buffer makes imm_path_add() fail, which trellis_unzip()
 * reports as DCP_ENOMEM.
 */
#ifndef IMM_PATH_H
#define IMM_PATH_H

struct imm_step
{
  int state_id;
  int seqsize;
  float score;
};

struct imm_path
{
  int capacity;
  int nsteps;
  struct imm_step *steps;
};

static inline struct imm_step imm_step(int state_id, int seqsize, float score)
{
  return (struct imm_step){state_id, seqsize, score};
}

static inline int imm_path_add(struct imm_path *x, struct imm_step step)
{
  if (x->nsteps >= x->capacity) return 1;
  x->steps[x->nsteps++] = step;
  return 0;
}

static inline void imm_path_reverse(struct imm_path *x)
{
  for (int i = 0, j = x->nsteps - 1; i < j; ++i, --j)
  {
    struct imm_step t = x->steps[i];
    x->steps[i] = x->steps[j];
    x->steps[j] = t;
  }
}

#endif
