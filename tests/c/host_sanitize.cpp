// host_sanitize.cpp -- TEST INFRASTRUCTURE: the host-side .dcp reader, windows, partitions, one short window walk, a
// few memory plans of the path pass, a few hundred plans of window lists and the code rows of short reads under ASan + UBSan, on the golden database, on truncated copies and on 200 randomly corrupted copies (must fail
// cleanly, never fault).
#include "deciphon_hip.h"
#include "deciphon_host.h"
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char **argv)
{
  struct dcp_db *db = NULL;
  int rc = dcp_db_open(argv[1], &db);
  if (rc) { printf("open rc %d\n", rc); return 1; }
  int n = dcp_db_num_proteins(db);
  printf("proteins %d\n", n);
  for (int i = 0; i < n; ++i)
  {
    int K = 0;
    rc = dcp_db_protein_core_size(db, i, &K);
    char acc[32];
    float *tr = (float *)malloc((K + 1) * 7 * 4), *em = (float *)malloc((size_t)(K + 1) * 1364 * 4), *bm = (float *)malloc(K * 4);
    float nul[1364], bg[1364];
    char *cons = (char *)malloc(K + 1);
    rc = dcp_db_read_protein(db, i, tr, em, bm, nul, bg, acc, cons);
    printf("  %d K=%d acc=%s rc=%d\n", i, K, acc, rc);
    free(tr); free(em); free(bm); free(cons);
  }
  struct dcp_window w;
  dcp_window_setup(&w, 10000, 173);
  while (dcp_window_next(&w)) printf("  window %d [%d,%d)\n", w.idx, w.start, w.stop);
  for (int N = 0; N < 30; ++N) for (int P = 1; P < 9; ++P) { long s = 0; for (int i = 0; i < P; ++i) s += dcp_partition_size(N, P, i); if (s != N) { printf("partition bug\n"); return 1; } }
  dcp_db_close(db);
  {
    /* a short walk (csrc/scan_walk.h): 2 profiles x 4 reads in one chunk; every third window passes the filter, and
     * every second path holds a hit that ends in the middle of its window */
    int32_t const K[2] = {3, 12}, R[4] = {0, 700, 2000, 700}, chunk[4] = {0, 2, 0, 4};
    int64_t nw = 0;
    for (int p = 0; p < 2; ++p) for (int s = 0; s < 4; ++s) nw += dcp_window_count(R[s], K[p]);
    struct dcp_scan_walk *walk = dcp_scan_walk_new(2, K, 4, R);
    std::vector<dcp_hip_window> wins((size_t)nw);
    std::vector<int64_t> base(2 * 4 + 1);
    rc = dcp_scan_walk_chunk_windows(walk, chunk, nw, wins.data(), base.data());
    if (rc) { printf("walk: chunk_windows rc %d\n", rc); return 1; }
    std::vector<int32_t> idx;
    std::vector<float> lrt;
    for (int64_t i = 0; i < nw; i += 3) { idx.push_back((int32_t)i); lrt.push_back((float)i); }
    dcp_scan_walk_chunk_scored(walk, chunk, base.data(), (int)idx.size(), idx.data(), lrt.data());
    long nhits = 0, rounds = 0;
    while (dcp_scan_walk_waiting(walk, 0) || dcp_scan_walk_waiting(walk, 1))
    {
      dcp_hip_window const *w = NULL;
      dcp_walk_hit const *hits = NULL;
      int64_t n = dcp_scan_walk_take(walk, 1, &w);
      std::vector<uint8_t> is_hit((size_t)n);
      std::vector<int32_t> pos((size_t)n);
      for (int64_t i = 0; i < n; ++i) { is_hit[(size_t)i] = (w[i].start / 7) % 2; pos[(size_t)i] = (w[i].stop - w[i].start) / 2; }
      if (n) nhits += (long)dcp_scan_walk_path_walked(walk, is_hit.data(), pos.data(), &hits);
      n = dcp_scan_walk_take(walk, 0, &w);
      idx.clear(); lrt.clear();
      for (int64_t i = 0; i < n; i += 3) { idx.push_back((int32_t)i); lrt.push_back(1.0f); }
      dcp_scan_walk_cost_scored(walk, (int)idx.size(), idx.data(), lrt.data());
      if (++rounds > 100000) { printf("walk does not end\n"); return 1; }
    }
    printf("walk done: %lld of %lld windows, %ld hits, %lld scored again\n", (long long)dcp_scan_walk_windows(walk),
           (long long)nw, nhits, (long long)dcp_scan_walk_take_queued(walk));
    dcp_scan_walk_del(walk);
  }
  {
    /* memory plans of the path pass (csrc/path_plan.h), cases of tests/test_path_plan.py: strip windows of K = 4200 and
     * 8192 and two short profiles, both kinds, every B, budgets around a whole table, a chunk cap, overrides; every
     * placement holds its checkpoints and its scratch */
    int32_t const L[5] = {120, 120, 3000, 600, 2000}, K[5] = {4200, 300, 4200, 8192, 1000}, Kp[5] = {6144, 384, 6144, 8192, 1024};
    int32_t const W[5] = {8, 1, 8, 8, 4}, Bs[4] = {0, 5, 50, 500};
    uint8_t const strip[5] = {1, 0, 1, 1, 0};
    int64_t const budgets[5] = {1, 8924960, 8924959, (int64_t)64 << 20, (int64_t)200 << 20}, chunks[3] = {0, 40000000, (int64_t)2 << 30};
    long plans = 0;
    for (int kind = 0; kind < 2; ++kind) for (int b = 0; b < 4; ++b) for (int m = 0; m < 5; ++m) for (int c = 0; c < 3; ++c)
      for (int strict = 0; strict < 2; ++strict) for (int over = 0; over < 8; over += 3)
      {
        int32_t inb[5], nb[5], rows[5];
        int64_t ck[5], scr[5], bytes[5];
        int G = 0, blocked = 0;
        rc = dcp_path_plan_of(kind, 5, L, K, Kp, W, strip, Bs[b], budgets[m], strict, chunks[c], over, inb, nb, rows, ck, scr,
                              bytes, &G, &blocked);
        if (rc || G < 1) { printf("plan rc %d G %d\n", rc, G); return 1; }
        for (int i = 0; i < 5; ++i)
          if (ck[i] > bytes[i] || scr[i] + (int64_t)rows[i] * 3 * K[i] * 4 > bytes[i] || (kind == 0 && (scr[i] || rows[i])))
          { printf("plan: window %d leaves its placement\n", i); return 1; }
        ++plans;
      }
    if (dcp_path_plan_of(2, 0, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0) return 1;
    printf("plan done: %ld plans\n", plans);
  }
  {
    /* plans of small random window lists (csrc/stage_plan.h) and the launches of their cost passes, on tables of this
     * program's own: 7 profiles (the last outside every class), 5 reads, lists ascending by profile and not, every
     * arena kind and switch, windows that are refused; the lists of a plan stay inside what it says they hold */
    int32_t const prof[7][5] = {{3, 64, 0, 0, 0}, {14, 64, 0, 0, 3}, {100, 128, 1, 0, 10}, {300, 384, 4, 1, -1},
                                {350, 384, 4, 0, -1}, {5000, 6144, 11, 0, -1}, {20000, 20480, -1, 0, -1}};
    int32_t shapes[11][2];
    for (int s = 0; s < 11; ++s) { shapes[s][0] = s < 3 ? 16 : s < 5 ? 8 : s < 8 ? 4 : 2; shapes[s][1] = s < 8 ? 1 + s % 4 : 0; }
    int64_t const seq_off[6] = {0, 40, 41, 141, 142, 400}, row_off[6] = {0, 41, 43, 144, 146, 405};
    long plans = 0, refusals = 0;
    srand(7);
    for (int it = 0; it < 400; ++it)
    {
      int const nw = rand() % 60, arena = it % 3 == 0 ? rand() % 3 : 0;
      std::vector<dcp_hip_window> wins((size_t)nw);
      std::vector<int64_t> addr((size_t)nw);
      for (int i = 0; i < nw; ++i)
      {
        int const bad = rand() % 300; /* now and then a window that is refused, or the profile that is */
        dcp_hip_window &v = wins[(size_t)i];
        v.profile = it % 2 ? rand() % 6 : i * 6 / nw;
        v.seq = rand() % 5;
        int const len = (int)(seq_off[v.seq + 1] - seq_off[v.seq]);
        v.start = len ? rand() % len : 0;
        v.stop = v.start + (len - v.start ? 1 + rand() % (len - v.start) : 0);
        if (bad == 0) v.profile = rand() % 2 ? -1 : 7;
        if (bad == 1) v.seq = rand() % 2 ? -1 : 5;
        if (bad == 2) v.stop = len + 1;
        if (bad == 3) v.stop = v.start;
        if (bad == 4) v.profile = 6;
        addr[(size_t)i] = 4096 + 512 * (int64_t)i;
      }
      int64_t sizes[3] = {0, 0, 0};
      int32_t cb[13], cw[12], cp[24], pk[12], pg[12], xt = 0;
      double cells = 0;
      int64_t arena_bytes = 0;
      char const *what = NULL;
      rc = dcp_stage_plan_of(nw, wins.data(), 7, &prof[0][0], 5, seq_off, row_off, arena, addr.data(), it % 5 != 0, it % 7 != 0,
                             &shapes[0][0], sizes, NULL, NULL, NULL, cb, cw, cp, pk, pg, &cells, &arena_bytes, &xt, &what);
      if (rc) { if (!what || !what[0]) { printf("stage: refusal %d without a message\n", rc); return 1; } ++refusals; ++plans; continue; }
      std::vector<int64_t> problems((size_t)sizes[0] * 4), packs((size_t)sizes[1] * 33);
      std::vector<int32_t> groups((size_t)sizes[2] * 2);
      rc = dcp_stage_plan_of(nw, wins.data(), 7, &prof[0][0], 5, seq_off, row_off, arena, addr.data(), it % 5 != 0, it % 7 != 0,
                             &shapes[0][0], sizes, problems.data(), packs.data(), groups.data(), cb, cw, cp, pk, pg, NULL, NULL,
                             NULL, NULL);
      if (rc || cb[12] != sizes[0] || pk[11] != sizes[1] || pg[11] != sizes[2]) { printf("stage: rc %d, shares and sizes differ\n", rc); return 1; }
      for (int s = 0; s < 11; ++s)
        for (int g = pg[s]; g < pg[s + 1]; ++g)
          if (groups[2 * (size_t)g] < 0 || groups[2 * (size_t)g] + groups[2 * (size_t)g + 1] > pk[s + 1] - pk[s])
          { printf("stage: a group leaves its shape's packs\n"); return 1; }
      int32_t rows[36][6];
      for (int narrow = 0; narrow < 2; ++narrow)
      {
        int const nl = dcp_cost_schedule_of(cb, cw, cp, pk, pg, narrow, 36, &rows[0][0]);
        if (nl < 0 || nl > 36) { printf("schedule: %d launches\n", nl); return 1; }
        int64_t covered = 0;
        for (int i = 0; i < nl; ++i) covered += rows[i][0] >= 1 && rows[i][0] <= 3 ? rows[i][3] : 0;
        if (covered != sizes[0]) { printf("schedule: %lld of %lld problems launched\n", (long long)covered, (long long)sizes[0]); return 1; }
      }
      ++plans;
    }
    if (!refusals || refusals == plans) { printf("stage: %ld refusals of %ld\n", refusals, plans); return 1; }
    printf("stage done: %ld plans\n", plans);
  }
  {
    /* code rows (csrc/code_rows.h, the host's use of it) of reads of 0..7 nucleotides, every count of symbols below
     * five to the left of a row, into buffers of exactly their size: the minus rows are the plus rows of the read
     * reverse-complemented here, and word 0 of a plus row is the nucleotide in front of it */
    srand(11);
    for (int len = 0; len <= 7; ++len)
    {
      std::vector<uint8_t> nt((size_t)len), rev((size_t)len);
      for (int i = 0; i < len; ++i) nt[(size_t)i] = (uint8_t)(rand() & 3);
      for (int i = 0; i < len; ++i) rev[(size_t)i] = (uint8_t)(3 - nt[(size_t)(len - 1 - i)]);
      std::vector<uint32_t> plus(((size_t)len + 1) * 8), minus(plus.size()), rev_plus(plus.size());
      if (dcp_code_rows_of(nt.data(), len, 0, plus.data()) || dcp_code_rows_of(nt.data(), len, 1, minus.data()) ||
          dcp_code_rows_of(rev.data(), len, 0, rev_plus.data()))
      { printf("code rows: refused at length %d\n", len); return 1; }
      if (minus != rev_plus) { printf("code rows: minus rows differ at length %d\n", len); return 1; }
      for (int r = 0; r <= len; ++r)
        if (plus[(size_t)r * 8] != (r ? nt[(size_t)r - 1] : 0u) || plus[(size_t)r * 8 + 5] || plus[(size_t)r * 8 + 7])
        { printf("code rows: row %d of length %d\n", r, len); return 1; }
    }
    printf("code rows done: lengths 0..7\n");
  }
  /* truncated and corrupt files must fail cleanly */
  FILE *f = fopen(argv[1], "rb"); fseek(f, 0, SEEK_END); long sz = ftell(f); fseek(f, 0, SEEK_SET);
  char *buf = (char *)malloc(sz); fread(buf, 1, sz, f); fclose(f);
  long cuts[] = {0, 1, 10, 100, 1000, sz / 2, sz - 1};
  for (unsigned c = 0; c < sizeof cuts / sizeof *cuts; ++c)
  {
    f = fopen(argv[2], "wb"); fwrite(buf, 1, cuts[c], f); fclose(f);
    rc = dcp_db_open(argv[2], &db);
    printf("  truncated at %ld: rc %d\n", cuts[c], rc);
    if (!rc) { int m = dcp_db_num_proteins(db); for (int i = 0; i < m; ++i) { int K; (void)dcp_db_protein_core_size(db, i, &K); (void)dcp_db_read_protein(db, i, 0, 0, 0, 0, 0, 0, 0); } dcp_db_close(db); }
  }
  srand(1);
  for (int it = 0; it < 200; ++it)
  {
    char *c2 = (char *)malloc(sz); memcpy(c2, buf, sz);
    for (int j = 0; j < 8; ++j) c2[rand() % (it < 100 ? 2000 : sz)] = (char)rand();
    f = fopen(argv[2], "wb"); fwrite(c2, 1, sz, f); fclose(f); free(c2);
    rc = dcp_db_open(argv[2], &db);
    if (!rc) { int m = dcp_db_num_proteins(db); for (int i = 0; i < m && i < 3; ++i) { int K; if (!dcp_db_protein_core_size(db, i, &K) && K > 0 && K < 100000) { float *em = (float *)malloc((size_t)(K + 1) * 1364 * 4); float *tr = (float *)malloc((size_t)(K + 1) * 7 * 4); float *bm = (float *)malloc((size_t)K * 4); char *cons = (char *)malloc(K + 1); char acc[32]; (void)dcp_db_read_protein(db, i, tr, em, bm, 0, 0, acc, cons); free(em); free(tr); free(bm); free(cons); } } dcp_db_close(db); }
  }
  {
    /* a value nested a few hundred thousand arrays deep behind the first "idx" key (skipped by the reader):
     * must fail with an error code, not overflow the stack */
    char const key[] = {(char)0xa3, 'i', 'd', 'x'};
    long at = -1;
    for (long i = 0; i + 4 < sz && i < 4096; ++i) if (!memcmp(buf + i, key, 4)) { at = i + 4; break; }
    if (at < 0) { printf("no idx key\n"); return 1; }
    long const deep = 400000;
    char *c2 = (char *)malloc(at + deep); memcpy(c2, buf, at); memset(c2 + at, 0x91, deep);
    f = fopen(argv[2], "wb"); fwrite(c2, 1, at + deep, f); fclose(f); free(c2);
    rc = dcp_db_open(argv[2], &db);
    printf("  nested arrays: rc %d\n", rc);
    if (!rc) { printf("nested arrays accepted\n"); return 1; }
  }
  printf("fuzz done\n");
  free(buf);
  return 0;
}
