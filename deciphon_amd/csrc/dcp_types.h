// dcp_types.h -- plain structs shared by host code, HIP kernels and the wave emulator.
#pragma once
#include <stdint.h>

#define DCP_TABLE_SIZE 1364  // 4+16+64+256+1024 quasi-codon codes, c-core/viterbi.c:13
#define DCP_NUM_TRANS 8      // BM MM MI MD IM II DM DD, c-core/viterbi.h:22-32
#define DCP_NUM_XTRANS 13    // RR SN NN SB NB EB JB EJ JJ EC CC ET CT, c-core/viterbi.h:4-19
#define DCP_XT_STRIDE 16     // floats per row of the special-transition table
#define DCP_REF_LANES 8      // SIMD width of the reference build whose E tie rule is reproduced (-mavx2)
#define DCP_MODEL_MAX 16384  // c-core/model.h:12
#define DCP_NUM_CLASSES 12      // kernel classes by padded size (viterbi_kernels.h dcp_class_of)
#define DCP_STRIP_CLASS 11      // K > 4096: strips of DCP_STRIP_POSITIONS, state ring in HBM (StripWave)
#define DCP_NUM_PACK_SHAPES 11  // shapes of the packed cost kernels (viterbi_kernels.h dcp_pack_shape_of)

enum { DCP_BM, DCP_MM, DCP_MI, DCP_MD, DCP_IM, DCP_II, DCP_DM, DCP_DD };
enum { DCP_RR, DCP_SN, DCP_NN, DCP_SB, DCP_NB, DCP_EB, DCP_JB, DCP_EJ, DCP_JJ, DCP_EC, DCP_CC, DCP_ET, DCP_CT };

// One sequence position: codes of the 1..5-mers that END at this position,
// i.e. code_fn(pos - t, t) for t = 1..5 in c[t-1] (0 where the t-mer would start
// before the sequence).  32 bytes, one code per dword, so that a DP row costs one
// scalar dwordx8 load and no unpacking.
struct DcpCodeRow
{
  uint32_t c[8];
};

#define DCP_SP_STRIDE 8 // floats per row of special-state values in a DP table: N,B,J,E,C,0,0,0
#define DCP_ROW_HDR 4    // floats in front of every emission row: null[c], bg[c], 0, 0
#define DCP_MAX_STRIPS 8 // K > 4096: strips of 2048 positions (StripWave), up to 16384 padded positions

// A profile resident in HBM, in DP-parameter space (costs = -log-prob, +inf =
// impossible), padded to Kp = 64*Q*W positions with +inf.  All arrays live in
// one device pool of floats; the fields are offsets into it (in floats), so that
// kernels address them as kernel-argument base + scalar offset.
//   rows : 1364 emission rows, code-major, each DCP_ROW_HDR + Kp floats:
//          { null[c], bg[c], 0, 0, match[c][0..Kp) } -- everything a DP row needs
//          for one emission length sits behind ONE scalar offset c * stride
//   trans: [8][Kp]
//   cost_rows: the same rows in the order the cost kernel of shape cost_shape reads them (dcp_cost_order_col,
//          host_logic.h), [1364][DCP_COST_ORDER_HDR + 64 Q' W']; offset 0 = no copy, every kernel reads `rows`
struct DcpProfileDev
{
  int32_t K;         // core size
  int32_t Kp;        // padded positions
  int32_t Q;         // positions per lane
  int32_t W;         // waves per problem (1 for K <= 256)
  int64_t rows_off;  // [1364][DCP_ROW_HDR + Kp]
  int64_t trans_off; // [8][Kp]
  int64_t cost_rows_off; // 0 or [1364][dcp_cost_order_stride(Q', W')]
  int64_t cost_shape;    // DCP_COST_SHAPE(Q', W') of the kernel the copy is for
};
#define DCP_COST_SHAPE(Q, W) ((Q) * 256 + (W))
#define DCP_COST_ORDER_HDR 32 // floats in front of the columns of a cost-order row: { null, bg, 0, 0 }, +inf to 128 bytes
#ifdef __HIPCC__
#define DCP_HDI __host__ __device__ inline
#else
#define DCP_HDI inline
#endif
// c-core/lrt.h:6-9, in its fp32 operations: the score of a window, for the host and for the kernels that filter and fit
// by it (dcp_lrt_filter_kernel, dcp_calib_gather_kernel)
DCP_HDI float dcp_lrt(float null_loglik, float alt_loglik) { return -2 * (null_loglik - alt_loglik); }

// where position k of a profile lies among the columns of a cost-order row of shape (Q, W) -- the map itself is
// described at host_logic.h, "the cost-order copy"; stated here, once, for the host and for the kernel that writes the
// copy on the device (press_rows.hip)
DCP_HDI int dcp_cost_order_col(int Q, int W, int k)
{
  (void)W;
  int const g = k / Q, q = k % Q, w = g / 64, e = g % 64, c = q / 4;
  int const wc = Q - 4 * c < 4 ? Q - 4 * c : 4;
  return 64 * Q * w + 256 * c + e * wc + (q - 4 * c);
}
DCP_HDI int dcp_cost_order_stride(int Q, int W) { return DCP_COST_ORDER_HDR + 64 * Q * W; }

// One (profile x sequence-window) DP problem.
struct DcpProblem
{
  int32_t profile;  // index into the DcpProfileDev array
  int32_t L;        // window length
  int64_t code_row; // index of the window's position 0 in the DcpCodeRow array (row l of the DP reads code_row + l)
  int32_t xt_row;   // row of the special-transition table = max(L/3, 1), c-core/thread.c:112
  int32_t out;      // slot in the output arrays
  int64_t trellis;  // path pass: offset (in bytes) of this problem's trellis in the arena
};

// Up to 16 windows of ONE profile that share a wavefront (viterbi_pack.h): group g of the wave runs window g.
// L[g] = 0 marks an idle group.  code_row is an index into the DcpCodeRow array (the array stays below 2^32 rows).
struct DcpPack
{
  int32_t profile;
  int32_t Lmax;          // the longest window of the pack: the row loop runs to it
  int32_t L[16];
  int32_t xt_row[16];    // max(L / 3, 1), c-core/thread.c:112
  int32_t out[16];       // slot in the output arrays
  uint32_t code_row[16]; // index of the window's position 0 in the DcpCodeRow array
};

// ---- fast path pass in blocks (checkpoint + recompute) -------------------------------------------------
// A window's DP table (12 B per cell) is never held whole.  A first pass (the cost kernel) leaves the FOLDED ring
// of five rows -- Mpre[5][Kp], Ipre[5][Kp], Spre[5] and X per lane -- every B rows (B a multiple of 5): checkpoint j is the
// state after row j * B.  Blocks are then taken from the last to the first: block j is recomputed from checkpoint
// j (block 0 from row 0) over rows j*B + 1 .. min(L, (j+1)*B + 5) into a table of B + 6 rows (row l at slot
// l - j*B), and the traceback walks the part of the path whose stage lies in (j*B + 5, (j+1)*B + 5] -- every
// row it reads there, stage - 5 .. stage, is in the block's table -- before handing over to block j - 1.
#define DCP_CKPT_ROWS_DEFAULT 500
#define DCP_CKPT_SP 6 // lane rows of specials per checkpoint: Spre[5], X
DCP_HDI long long dcp_ckpt_floats(int Kp, int W) { return 10LL * Kp + (long long)DCP_CKPT_SP * 64 * W; } // W waves per window
// the strip class (K > 4096, StripWave) cannot fold B of a row into its ring -- rest[5][Kp], Ipre[5][Kp] -- and saves
// B of the five rows behind the lane rows (padded to 32 bytes)
DCP_HDI long long dcp_strip_ckpt_floats(int Kp, int W) { return dcp_ckpt_floats(Kp, W) + 8; }

// blocks of a window of L rows with checkpoints every B rows (B = 0: one block, the whole window)
DCP_HDI int dcp_num_blocks(int L, int B) { return B <= 0 || L <= B + 5 ? 1 : (L - 5 + B - 1) / B; }

// rows a block's table holds, the row the block starts from included (row 0 for block 0)
DCP_HDI int dcp_block_slots(int L, int B) { return (B <= 0 || L <= B + 5 ? L : B + 5) + 1; }

// floats of one block's table: specials[slots][DCP_SP_STRIDE] + cells[slots][3][Kp]
DCP_HDI long long dcp_block_table_floats(int L, int Kp, int B)
{
  return (long long)dcp_block_slots(L, B) * (DCP_SP_STRIDE + 3LL * Kp);
}

// Checkpoint j, the state after row j * B, exists iff block j does: j * B + 5 < L.  Is the state after row l one?
DCP_HDI bool dcp_ckpt_after(int L, int B, int l) { return B > 0 && l % B == 0 && l + 5 < L; }
DCP_HDI int dcp_ckpt_slot(int j) { return j - 1; } // where checkpoint j lies among a window's checkpoints

// Block j of a window as the comment above has it, in rows of the window.  Everything that computes, walks or replays a
// block -- the kernels, the host and the wave emulator (tests/emul) -- takes these from here and holds no such
// arithmetic of its own.  B = 0 is the one block that is the whole window.
struct DcpBlock
{
  int row_base; // the row it starts from, j * B: row l lies at slot l - row_base of the table
  int last;     // the last row it computes: row_base + B + 5, clamped to L
  int lo;       // the traceback hands over to block j - 1 at the first stage <= lo = row_base + 5; -1 for block 0
  int first;    // the first row the replay serves (row_replay.h), lo + 1: the traceback's partition; 0 for block 0
  int ckpt;     // slot of the checkpoint it starts from among the window's checkpoints; -1 for block 0 (from row 0)
  int slots;    // dcp_block_slots: its table is specials[slots][DCP_SP_STRIDE], then cells[slots][3][Kp]
};
DCP_HDI DcpBlock dcp_block(int L, int B, int j)
{
  DcpBlock b;
  b.slots = dcp_block_slots(L, B);
  b.row_base = j * B;
  b.last = L - b.row_base < b.slots ? L : b.row_base + b.slots - 1;
  b.lo = j > 0 ? b.row_base + 5 : -1;
  b.first = b.lo + 1;
  b.ckpt = dcp_ckpt_slot(j);
  return b;
}

// G blocks of a window are computed side by side into G tables, dcp_block_table_floats apart, the last blocks first:
// the block that launch `it` gives to table `sub`, negative when the window has none left for it ...
DCP_HDI int dcp_group_block(int L, int B, int G, int it, int sub) { return dcp_num_blocks(L, B) - 1 - (it * G + sub); }
// ... and where that table lies behind the first, in floats
DCP_HDI long long dcp_group_table(int L, int Kp, int B, int sub) { return sub * dcp_block_table_floats(L, Kp, B); }

// rows of the trellis that the replay of one block can serve (row_replay.h): B + 5 and row 0, for block 0
DCP_HDI int dcp_replay_block_rows(int B) { return B + 6; }

// The replay of launch `it` (row_replay.h): thread r of a window takes row *row of the block in table *sub -- a table's
// worth of threads per table, the last six of which have no row in a block above block 0.  False: no row for thread r.
DCP_HDI bool dcp_replay_thread_row(int L, int B, int G, int it, int r, int *sub, DcpBlock *blk, int *row)
{
  int const per = dcp_block_slots(L, B);
  *sub = r / per;
  if (*sub >= G) return false;
  int const j = dcp_group_block(L, B, G, it, *sub);
  if (j < 0) return false;
  *blk = dcp_block(L, B, j);
  *row = blk->first + r % per;
  return *row <= blk->last;
}

// ---- which columns of an emission row a lane reads --------------------------------------------------------
// A profile of K positions is padded with +inf to Kp columns, and a lane whose positions all lie at or beyond K owns
// nothing: BM, MM, IM and DM are +inf there, so its Mpre is +inf from row 0 on and M = min_t(Mpre + em) is +inf
// whatever em holds, +inf or not; I, D and E never see em.  Such a lane does not fetch its padding columns.  It reads
// what the LAST lane that owns a position reads -- a line that lane fetches anyway -- and a lane that owns at least
// one position reads exactly its own Q columns, the +inf tail of the lane that straddles K included.
//   DCP_ROW_CANON       one wavefront of 64 lanes x Q positions on the canonical rows, chunk c = floats 4c .. of the
//                       lane (Q <= 4, and the table-writing kernels: one chunk of Q floats)
//   DCP_ROW_COST_ORDER  the same on the cost-order copy (cost_rows_off): the clamp holds chunk by chunk
//   DCP_ROW_PACK        a group of S lanes (viterbi_pack.h): lane 0 is the separator and reads the row's header,
//                       offset 0; lane e >= 1 owns positions (e - 1) Q ..; the last real lane is the group's own
enum { DCP_ROW_CANON, DCP_ROW_COST_ORDER, DCP_ROW_PACK };
#define DCP_ROW_MAX_CHUNKS 3 // (Q + 3) / 4 for Q <= 10 (ten positions per lane: 4 + 4 + 2)

// lanes, of `lanes` that own Q positions each, with at least one position below K
DCP_HDI int dcp_row_real_lanes(int Q, int lanes, int K)
{
  int const n = (K + Q - 1) / Q;
  return n < 1 ? 1 : n > lanes ? lanes : n;
}
// the position-owning lane whose columns position-owning lane `lane` reads
DCP_HDI uint32_t dcp_row_source_lane(uint32_t real, uint32_t lane) { return lane < real ? lane : real - 1u; }
DCP_HDI int dcp_row_chunk_width(int Q, int c) { return Q - 4 * c < 4 ? Q - 4 * c : 4; }
// byte offset inside a row of chunk c of position-owning lane `lane` (lane = 64 w + e beyond one wavefront)
DCP_HDI uint32_t dcp_row_lane_bytes(int layout, int Q, uint32_t lane, int c)
{
  if (layout == DCP_ROW_COST_ORDER) // contiguous spans of 64 lanes x chunk width behind a 128-byte header
    return (uint32_t)(4 * DCP_COST_ORDER_HDR) + (lane >> 6) * (uint32_t)(256 * Q) + (uint32_t)(1024 * c) +
           (lane & 63u) * (uint32_t)(4 * dcp_row_chunk_width(Q, c));
  return (uint32_t)(DCP_ROW_HDR * 4) + lane * (uint32_t)(Q * 4) + (uint32_t)(16 * c);
}
// The statement itself: lanes of the shape that own a real position of a profile of K positions, and where lane e
// (of the wavefront, or of its group of S) reads chunk c of an emission row.  The kernels take the three functions
// above (CostWave::init, PackWave::init); the host and the tests take this one.
DCP_HDI int dcp_row_read_lanes(int layout, int Q, int S, int K)
{
  return dcp_row_real_lanes(Q, layout == DCP_ROW_PACK ? S - 1 : 64, K);
}
DCP_HDI uint32_t dcp_row_read_offset(int layout, int Q, int S, int K, uint32_t e, int c)
{
  uint32_t const real = (uint32_t)dcp_row_read_lanes(layout, Q, S, K);
  if (layout != DCP_ROW_PACK) return dcp_row_lane_bytes(layout, Q, dcp_row_source_lane(real, e), c);
  return e == 0 ? 0u : dcp_row_lane_bytes(DCP_ROW_CANON, Q, dcp_row_source_lane(real, e - 1u), 0);
}

// ---- which XCD's L2 serves which windows of a cost launch ----------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs, each with its own 4 MiB L2: with the plain blockIdx -> problem
// mapping the windows of one profile (neighbours in the profile-sorted list) land on all eight L2s, and every L2 holds
// the table of every profile in flight.  The eighths give XCD x the x-th contiguous eighth of the list instead (the
// bijective form for any n), so an L2 sees an eighth of the profiles.  A speed choice only: nothing depends on where a
// workgroup runs.
#define DCP_NUM_XCDS 8
#define DCP_XCD_L2_BYTES (4LL << 20)
DCP_HDI int dcp_xcd_eighths_entry(int b, int n)
{
  int const q = n >> 3, r = n & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}
enum { DCP_PLACE_AUTO = -1, DCP_PLACE_PLAIN = 0, DCP_PLACE_EIGHTHS = 1 };
// tables that meet in one L2 when `resident` workgroups, neighbours in a list of `windows_per_profile` windows of
// each of `nprofiles` profiles, run beside each other: the run of a list that long touches that many profiles
DCP_HDI long long dcp_xcd_tables_in_l2(long long resident, int windows_per_profile, int nprofiles)
{
  long long const t = resident / windows_per_profile + 1;
  return t < nprofiles ? t : nprofiles;
}
// The rule, per launch of a cost kernel whose list is in profile order (a window's time depends on L alone there, so
// the eighths are even in time): `workgroups` windows, `windows_per_profile` of them on average per profile,
// `table_bytes` of emission rows per profile that the kernel reads, `resident_per_xcd` workgroups that one XCD holds
// at the occupancy the kernel was compiled for.  In plain order the resident workgroups of the whole chip are one run
// of the list and every L2 serves all its tables; in eighths an L2 serves the tables of its own XCD's run.  Eighths
// when the former do not fit an L2 and the latter are fewer.
DCP_HDI int dcp_xcd_placement(int workgroups, int windows_per_profile, long long table_bytes, int resident_per_xcd)
{
  if (workgroups < 1 || windows_per_profile < 1 || resident_per_xcd < 1) return DCP_PLACE_PLAIN;
  int const nprofiles = (workgroups + windows_per_profile - 1) / windows_per_profile;
  long long const plain = dcp_xcd_tables_in_l2((long long)DCP_NUM_XCDS * resident_per_xcd, windows_per_profile, nprofiles);
  long long const eighths = dcp_xcd_tables_in_l2(resident_per_xcd, windows_per_profile, nprofiles);
  return plain * table_bytes > DCP_XCD_L2_BYTES && eighths < plain ? DCP_PLACE_EIGHTHS : DCP_PLACE_PLAIN;
}

// where the traceback of one window stands between blocks (all zero = not started)
struct DcpTraceState
{
  int32_t state;  // state id to visit next (c-core/state.h:9-25)
  int32_t stage;  // its DP row
  int32_t status; // 0 = under way, 1 = finished, < 0 = DCP_TB_*
  int32_t pad;
  int64_t n;      // steps written so far (from the end of the step buffer backwards)
};
