// lane_cases.h -- TEST INFRASTRUCTURE ONLY.
// The lane vocabulary op by op: small cases written against the names of deciphon_amd/csrc/lane_ops_gpu.h alone, as
// viterbi_body.h is, and instantiated twice -- lane_conf.hip on the GPU's own vocabulary, lane_conf_emul.cpp on the
// wave emulator's (tests/emul/lane_ops_emul.h).  tests/test_gpu_lane_ops.py feeds both the same words and compares
// every output word; tests/test_lane_ops_emul.py holds the emulator's side against plain numpy.
//
// A case is a struct with W (wavefronts of its group: it runs on 64 W lanes) and run(io).  What it reads and writes
// goes through `io`, which each instantiation provides before it includes this file:
//   io.f(j) / io.u(j)            per-lane input vector j, as lf / lu
//   io.of / ou / om (j, x)       per-lane output vector j from an lf / lu / lm (a predicate is written as 0 or 1)
//   io.osf / osu / osb (j, x)    a uniform result (float / uint32_t / bool): written to every lane of output j, so a
//                                value that is not uniform on the GPU shows
//   io.os64(j, x)                a 64-bit uniform result, low word to output j, high word to j + 1
//   io.sf(s) / su(s) / si(s)     scalar s of this input vector (uniform)
//   io.mem() / memu()            read-only words shared by all vectors of the call
//   io.omem() / omemu()          this vector's own output words (the caller fills them; untouched words must stay)
//   io.lds(n)                    the first n words of mem() as an LDS table (the emulator: mem() itself)
// LANE_POLICY is the lane policy of traceback.h on that side (DcpLanesWave / DcpLanesHost).
//
// The table at the end lists every case: name, the vocabulary names it covers (the completeness guard of
// tests/test_lane_ops_emul.py reads them), inputs, outputs, type.  The assembly-bearing ops (wave_min, wave_minu,
// add_quad0_x5, pack_unstash_*) come in three contexts -- CTX 0 on a value the VALU wrote in the statement before,
// 1 on a freshly loaded value, 2 twice with the first result feeding the second -- because their hand-counted wait
// states must hold wherever the compiler places them.
#pragma once

#define LC_INF __builtin_inff()

// ---- elementwise ---------------------------------------------------------------------------------------------------
struct c_elem_f
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf const a = io.f(0), b = io.f(1), c = io.f(2);
    io.of(0, lmin(a, b));
    io.of(1, lmin(b, a));
    io.of(2, lmin3(a, b, c));
    io.of(3, lmin3(c, b, a));
    io.om(4, llt(a, b));
    io.om(5, leq(a, b));
    io.of(6, lsel(llt(a, b), a, c));
    io.of(7, lneg(a));
    io.of(8, a + b);
    io.of(9, lf_splat(io.sf(0)));
    io.of(10, lf_pin(io.sf(0)) + a);
    io.of(11, a + io.sf(0));
  }
};

struct c_elem_u
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lu const a = io.u(0), b = io.u(1);
    io.om(0, llt_u(a, b));
    io.om(1, lequ(a, b));
    io.ou(2, lselu(llt_u(a, b), a, b));
    io.ou(3, lminu(a, b));
    io.ou(4, lmaxu(a, b));
    io.ou(5, lane_shr(a, io.si(0)));
    io.ou(6, lu_splat(io.su(1)));
    io.ou(7, lane_ids());
    io.ou(8, a + b);
    // (predicates are combined from integer compares: the kernels are built with -fno-honor-nans, under which the
    // compiler may rewrite the negation of a float compare, and what that does with a NaN is nobody's contract)
    io.om(9, land(llt_u(a, b), lequ(a, io.u(2))));
    io.om(10, lor(llt_u(a, b), lequ(a, io.u(2))));
    io.om(11, lnot(lequ(a, b)));
  }
};

// ---- shifts --------------------------------------------------------------------------------------------------------
struct c_shift_up
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf const a = io.f(0), b = io.f(1);
    float const fill = io.sf(0);
    io.of(0, lane_shift_up(a, fill));
    io.of(1, lane_shift_up(a + b, fill));
    lf x = a;
    io.of(2, lane_shift_up_again(x));
    lf y = lane_shift_up(a + b, fill); // shifted before, then once more where it is needed
    io.of(3, lane_shift_up_again(y));
    io.of(4, y);
  }
};

// the kept register through 50 rows: lane 0 of `keep` is written by no shift and must still hold what it held
struct c_shift_keep
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf x = io.f(0), keep = io.f(1);
    lf const step = io.f(2);
    lf s = x;
    for (int r = 0; r < 50; ++r)
    {
      s = lane_shift_up_keep(x, keep);
      x = lmin(s + step, x);
    }
    io.of(0, s);
    io.of(1, keep);
    io.of(2, x);
  }
};

template <int W_> struct c_seg_shift
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    lf const a = io.f(0), b = io.f(1), fill = io.f(2);
    io.of(0, g.seg_shift_up(a, fill));
    io.of(1, g.seg_shift_up(a + b, fill));
    io.om(2, g.seg_first());
    io.om(3, g.last_lane());
    io.ou(4, g.lane);
  }
};

// ---- reductions and votes ------------------------------------------------------------------------------------------
template <int CTX> struct c_wave_min
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    if constexpr (CTX == 0)
      io.osf(0, wave_min(io.f(0) + io.f(1)));
    else if constexpr (CTX == 1)
      io.osf(0, wave_min(io.f(0)));
    else
    {
      float const m = wave_min(io.f(0));
      io.osf(0, m);
      io.osf(1, wave_min(lmin(io.f(1), lf_splat(m) + io.f(2))));
    }
  }
};

template <int CTX> struct c_wave_minu
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    if constexpr (CTX == 0)
      io.osu(0, wave_minu(io.u(0) + io.u(1)));
    else if constexpr (CTX == 1)
      io.osu(0, wave_minu(io.u(0)));
    else
    {
      uint32_t const m = wave_minu(io.u(0));
      io.osu(0, m);
      io.osu(1, wave_minu(lmaxu(io.u(1), lu_splat(m) + io.u(2))));
    }
  }
};

template <int CTX> struct c_add_quad0_x5
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf s[5], e[5], r[5];
    for (int t = 0; t < 5; ++t)
    {
      s[t] = io.f(t);
      e[t] = io.f(5 + t);
      if constexpr (CTX == 0)
      {
        s[t] = s[t] + io.f(10);
        e[t] = e[t] + io.f(10);
      }
    }
    add_quad0_x5(r, s, e);
    if constexpr (CTX == 2)
    {
      lf r2[5];
      add_quad0_x5(r2, s, r); // the first sums are the second's quad operand
      for (int t = 0; t < 5; ++t) io.of(5 + t, r2[t]);
    }
    for (int t = 0; t < 5; ++t) io.of(t, r[t]);
  }
};

template <int S> struct c_groups
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf const a = io.f(0), b = io.f(1);
    io.of(0, group_min<S>(a));
    io.of(1, group_min<S>(a + b));
    io.of(2, group_min01<S>(a));
    io.of(3, group_min01<S>(a + b));
    io.of(4, group_bcast0<S>(a));
    io.of(5, group_bcast0<S>(a + b));
    io.of(6, quad_bcast0(a));
    io.of(7, quad_bcast0(a + b));
  }
};

struct c_votes
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lm const m = lequ(io.u(0), lu_splat(1u));
    io.osb(0, wave_any(m));
    io.os64(1, wave_ballot(m));
    io.osf(3, read_lane(io.f(1), io.si(0)));
    io.osu(4, read_laneu(io.u(2), io.si(0)));
    io.osf(5, read_lane(io.f(1) + io.f(3), io.si(0)));
  }
};

// the lane policy of traceback.h: f is called with the lane index
struct c_lane_policy
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    uint32_t const *t = io.memu() + io.su(0);
    io.os64(0, LANE_POLICY::ballot([&](int lane) { return (t[lane] & 1u) != 0u; }));
    io.osu(2, (uint32_t)LANE_POLICY::max_of([&](int lane) { return (int)t[64 + lane]; }));
    if (LANE_POLICY::leader()) io.omemu()[0] = t[0];
  }
};

// ---- Group<W>: what crosses a wave boundary --------------------------------------------------------------------------
// W = 1: the calls are DPP / readlane and the put_* vanish; W > 1: LDS words published by put_*, consumed after sync()
template <int W_> struct c_group_exchange
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    lf const a = io.f(0), b = io.f(1), X = io.f(4);
    lu const ua = io.u(2);
    lm const m = lequ(io.u(3), lu_splat(1u));
    g.put_last(GS_M, a);
    g.put_min(GS_I, b);
    g.put_minu(GS_D, ua);
    g.put_any(GS_E, m);
    g.put_count(GS_F, m);
    g.put_lanes4(GS_X, X);
    g.sync();
    io.of(0, g.get_shift(GS_M, a, io.sf(0)));
    lf keep = lf_splat(LC_INF); // (beyond one wave the GPU takes +inf, which is what the kernels keep there)
    io.of(1, g.get_shift_keep(GS_M, a, keep));
    io.osf(2, g.get_min(GS_I, b));
    io.osu(3, g.get_minu(GS_D, ua));
    io.osb(4, g.get_any(GS_E, m));
    io.osu(5, (uint32_t)g.get_count(GS_F, m));
    for (int l = 0; l < 4; ++l) io.osf(6 + l, g.get_lane(GS_X, X, l));
    if constexpr (W_ > 1)
    {
      float N, J;
      g.get_nj(GS_X, X, N, J);
      io.osf(10, N);
      io.osf(11, J);
      io.of(12, g.get_shift_carry(GS_M, a, lf_splat(io.sf(0))));
      // seg_any is per wavefront on the GPU and over the whole group on the emulator (an extra lazy turn in a
      // converged wavefront changes nothing): u(5) is empty, or set in every wavefront, where the two agree
      io.osb(13, g.seg_any(lequ(io.u(5), lu_splat(1u))));
    }
  }
};

// the kept shift of one wave through Group<1>, 50 rows (W > 1 has no kept register: c_group_exchange)
struct c_group1_keep
{
  static constexpr int W = 1;
  Group<1> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    lf x = io.f(0), keep = io.f(1), s = x;
    for (int r = 0; r < 50; ++r)
    {
      s = g.get_shift_keep(GS_M, x, keep);
      x = lmin(s + io.f(2), x);
    }
    io.of(0, s);
    io.of(1, keep);
    io.ou(2, g.lane);
  }
};

// records of a row by parity; the strip's carry stands in front of wave 0
template <int W_> struct c_group_rec
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    g.sync();
    int const par = io.si(0);
    if (io.su(1) == 1u) g.put_carry(par, io.f(4), io.f(5), io.f(6));
    if (io.su(1) == 2u)
    {
      g.put_carry(par, io.f(4), io.f(5), io.f(6));
      g.sync();
      g.put_carry_inf(par);
    }
    g.put_rec(par, io.f(0), io.f(1), io.f(2), io.f(3));
    g.sync();
    lf Mp, Ip, Dp;
    g.get_prev(par, Mp, Ip, Dp);
    io.of(0, Mp);
    io.of(1, Ip);
    io.of(2, Dp);
  }
};

// E and the one-barrier decision of a row: f(0..Q-1) = DD, then m_last, i_last, d_last, m_all
template <int Q, int W_> struct c_group_tdd
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    lf DD[Q];
    for (int q = 0; q < Q; ++q) DD[q] = io.f(q);
    int const par = io.si(0);
    g.put_tdd(DD);
    g.put_rec(par, io.f(Q), io.f(Q + 1), io.f(Q + 2), io.f(Q + 3));
    g.sync();
    float E;
    bool could;
    g.get_e_could(par, E, could);
    io.osf(0, E);
    io.osb(1, could);
  }
};

// the same of a strip: s(1) = strip, sf(2) = the floor of what may still enter
template <int Q, int W_> struct c_group_tdd_strip
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    g.sync();
    lf DD[Q];
    for (int q = 0; q < Q; ++q) DD[q] = io.f(q);
    int const par = io.si(0), s = io.si(1);
    g.put_tdd_strip(s, DD);
    if (io.su(3) != 0u)
      g.put_carry(par, io.f(Q), io.f(Q + 1), io.f(Q + 2));
    else
      g.put_carry_inf(par);
    g.put_rec(par, io.f(Q), io.f(Q + 1), io.f(Q + 2), io.f(Q + 3));
    g.sync();
    float E;
    bool could;
    g.get_e_could_row(par, s, io.sf(2), E, could);
    io.osf(0, E);
    io.osb(1, could);
    lf Mp, Ip, Dp;
    g.get_prev(par, Mp, Ip, Dp);
    io.of(2, Dp);
  }
};

// ---- stashes -------------------------------------------------------------------------------------------------------
template <int Q, int W_> struct c_stash
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    lf v[Q], w[Q], r[Q];
    for (int q = 0; q < Q; ++q)
    {
      v[q] = io.f(q);
      w[q] = v[q] + io.f(Q);
    }
    g.template stash_q<Q, 8>(1, v);
    g.template stash_q<Q, 8>(6, w);
    g.template unstash_q<Q, 8>(6, r);
    for (int q = 0; q < Q; ++q) io.of(q, r[q]);
    g.template unstash_q<Q, 8>(1, r);
    for (int q = 0; q < Q; ++q) io.of(Q + q, r[q]);
    if constexpr (W_ == 1) // (a single wave takes its arrays back a few positions at a time)
    {
      constexpr int N = DcpStashChunk<Q>::N;
      for (int j = 0; j < Q / N; ++j)
      {
        lf c[N];
        g.template unstash_chunk<Q, 8>(6, j, c);
        for (int i = 0; i < N; ++i) io.of(2 * Q + N * j + i, c[i]);
      }
    }
  }
};

// f(6 a + ..): six arrays of Q
template <int Q, int CTX> struct c_pack_stash
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf in[6][Q], out[6][Q];
    for (int a = 0; a < 6; ++a)
      for (int q = 0; q < Q; ++q)
      {
        in[a][q] = io.f(a * Q + q);
        if constexpr (CTX == 0) in[a][q] = in[a][q] + io.f(6 * Q);
      }
    for (int a = 0; a < 6; ++a) pack_stash<Q>(a, in[a]);
    PackFold f;
    pack_unstash_issue(f);
    pack_unstash_wait<Q>(f, out[0], out[1], out[2], out[3], out[4], out[5]);
    if constexpr (CTX == 2)
    {
      for (int a = 0; a < 6; ++a) pack_stash<Q>(5 - a, out[a]); // what came back goes in again, the slots reversed
      PackFold f2;
      pack_unstash_issue(f2);
      pack_unstash_wait<Q>(f2, in[0], in[1], in[2], in[3], in[4], in[5]);
      for (int a = 0; a < 6; ++a)
        for (int q = 0; q < Q; ++q) io.of(6 * Q + a * Q + q, in[a][q]);
    }
    for (int a = 0; a < 6; ++a)
      for (int q = 0; q < Q; ++q) io.of(a * Q + q, out[a][q]);
  }
};

// ---- memory --------------------------------------------------------------------------------------------------------
template <int Q> struct c_load_store_q
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lu const lane = lane_ids();
    lf v[Q], w[Q];
    load_q<Q>(io.mem() + io.su(0), lane, v);
    for (int q = 0; q < Q; ++q)
    {
      io.of(q, v[q]);
      w[q] = io.f(q);
    }
    store_q<Q>(io.omem() + io.su(1), lane, w);
  }
};

// su(0) = bytes of the resource, su(1) = byte offset of the row
template <int Q> struct c_row_q
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    RowSrc const rows = rowsrc_make(io.mem(), io.su(0));
    float nil, bg;
    load_row_hdr(rows, io.su(1), nil, bg);
    io.osf(0, nil);
    io.osf(1, bg);
    lu const voff = row_lane_offset<Q>(lane_ids());
    io.ou(2, voff);
    lf v[Q];
    load_row_q<Q>(rows, voff, io.su(1), v);
    for (int q = 0; q < Q; ++q) io.of(3 + q, v[q]);
  }
};

// su(2) != 0: the cost-order layout
template <int Q, int W_> struct c_row_chunks
{
  static constexpr int W = W_;
  Group<W_> g;
  template <class IO> DCP_FN void run(IO &io)
  {
    g.init();
    RowSrc const rows = rowsrc_make(io.mem(), io.su(0));
    constexpr int N = DcpRowChunks<Q>::N;
    lu v[N];
    row_chunk_offsets<Q, W_>(g.lane, io.su(2) != 0u, v);
    for (int c = 0; c < N; ++c) io.ou(c, v[c]);
    lf out[Q];
    load_row_chunks<Q>(rows, v, io.su(1), out);
    for (int q = 0; q < Q; ++q) io.of(N + q, out[q]);
  }
};

// si(0) = Kp, su(1) = word offset of the code rows in memu(), su(2) = their number; u(0) = col_off, u(1) = code
template <int Q> struct c_pack_q
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    PackSrc const src = packsrc_make(io.mem(), io.si(0), reinterpret_cast<DcpCodeRow const *>(io.memu() + io.su(1)),
                                     io.su(2), io.u(0));
    lf v[Q];
    load_pack_q<Q>(src, io.u(1), v);
    for (int q = 0; q < Q; ++q) io.of(q, v[q]);
  }
};

// u(1) = the code row: rows at and past su(2) read 0
struct c_code_row
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    PackSrc const src = packsrc_make(io.mem(), io.si(0), reinterpret_cast<DcpCodeRow const *>(io.memu() + io.su(1)),
                                     io.su(2), io.u(0));
    lu code[5];
    load_code_row(src, io.u(1), code);
    for (int t = 0; t < 5; ++t) io.ou(t, code[t]);
  }
};

template <int Q> struct c_cols
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lf v[Q];
    load_cols<Q>(io.mem() + io.su(0), io.u(0), v);
    for (int q = 0; q < Q; ++q) io.of(q, v[q]);
  }
};

template <int N> struct c_lds
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lds_float const *t = io.lds(io.si(0));
    lf v[N];
    load_lds_q<N>(t, io.u(0), v);
    for (int q = 0; q < N; ++q) io.of(q, v[q]);
  }
};

// loads and stores by index: u(0) = any index into mem(), u(1) = distinct indices below 64, u(2) = who stores
struct c_lane_mem
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lu const lane = lane_ids();
    io.of(0, load_lane(io.mem(), io.u(0)));
    io.of(1, load_f32_at(io.mem(), io.u(0)));
    io.ou(2, load_u32_at(io.memu(), io.u(0)));
    store_lane(io.omem(), lane, io.f(3));
    store_f32_where(io.omem() + 64, io.u(1), lequ(io.u(2), lu_splat(1u)), io.f(4));
    store_sp_lane0(io.omem() + 128, lane, io.f(5), io.f(6), io.f(7), io.f(8), io.f(9));
    store_u32_lane0(io.omemu() + 136, lane, io.su(0));
    store_f32_lane0(io.omem() + 137, lane, io.sf(1));
  }
};

// si(0) = K, inside some lane's span
template <int Q> struct c_nodes
{
  static constexpr int W = 1;
  template <class IO> DCP_FN void run(IO &io)
  {
    lu w[Q];
    for (int q = 0; q < Q; ++q) w[q] = io.u(q);
    store_nodes_q<Q>(reinterpret_cast<uint16_t *>(io.omemu()), io.si(0), lane_ids(), w);
  }
};

// ---- the table: X(name, vocabulary names covered, per-lane inputs, outputs, type...) --------------------------------
#define LC_Q_ALL(X, M) M(X, 1) M(X, 2) M(X, 3) M(X, 4) M(X, 5) M(X, 6) M(X, 7) M(X, 8) M(X, 10)

#define LC_WAVE_MIN(X, C, WHAT) \
  X("wave_min/" WHAT, "wave_min", 3, 2, c_wave_min<C>) \
  X("wave_minu/" WHAT, "wave_minu", 3, 2, c_wave_minu<C>) \
  X("add_quad0_x5/" WHAT, "add_quad0_x5", 11, 10, c_add_quad0_x5<C>) \
  X("pack_stash<1>/" WHAT, "pack_stash pack_stash_mem pack_unstash_issue pack_unstash_wait", 7, 12, c_pack_stash<1, C>) \
  X("pack_stash<2>/" WHAT, "pack_stash pack_stash_mem pack_unstash_issue pack_unstash_wait", 13, 24, c_pack_stash<2, C>) \
  X("pack_stash<3>/" WHAT, "pack_stash pack_stash_mem pack_unstash_issue pack_unstash_wait", 19, 36, c_pack_stash<3, C>) \
  X("pack_stash<4>/" WHAT, "pack_stash pack_stash_mem pack_unstash_issue pack_unstash_wait", 25, 48, c_pack_stash<4, C>)

#define LC_GROUPS(X, S) \
  X("groups<" #S ">", "group_min group_min01 group_bcast0 quad_bcast0", 2, 8, c_groups<S>)

#define LC_EXCHANGE(X, W) \
  X("group_exchange<" #W ">", \
    "init sync put_last put_min put_minu put_any put_count put_lanes4 get_shift get_shift_keep get_shift_carry get_min " \
    "get_minu get_any get_count get_lane get_nj seg_any", \
    6, 14, c_group_exchange<W>)
#define LC_MULTI(X, W) \
  LC_EXCHANGE(X, W) \
  X("seg_shift<" #W ">", "seg_shift_up seg_first last_lane init", 3, 5, c_seg_shift<W>) \
  X("group_rec<" #W ">", "put_rec get_prev put_carry put_carry_inf", 7, 3, c_group_rec<W>)

#define LC_TDD(X, Q, W) \
  X("group_tdd<" #Q "," #W ">", "put_tdd put_rec get_e_could", Q + 4, 2, c_group_tdd<Q, W>)
#define LC_TDD_STRIP(X, Q, W) \
  X("group_tdd_strip<" #Q "," #W ">", "put_tdd_strip put_carry put_carry_inf put_rec get_e_could_row get_prev", Q + 4, 3, \
    c_group_tdd_strip<Q, W>)

#define LC_STASH(X, Q) \
  X("stash<" #Q ",1>", "stash_q unstash_q unstash_chunk dcp_stash dcp_unstash dcp_unstash_chunk dcp_stash_mem dcp_chunk_get", \
    Q + 1, 3 * Q, c_stash<Q, 1>) \
  X("stash<" #Q ",2>", "stash_q unstash_q dcp_stash dcp_unstash dcp_stash_mem dcp_chunk_get", Q + 1, 2 * Q, c_stash<Q, 2>)
#define LC_LOAD_STORE(X, Q) \
  X("load_store_q<" #Q ">", "load_q store_q", Q, Q, c_load_store_q<Q>) \
  X("row_q<" #Q ">", "rowsrc_make row_lane_offset load_row_hdr load_row_q", 0, 3 + Q, c_row_q<Q>)
#define LC_CHUNKS(X, Q) \
  X("row_chunks<" #Q ",1>", "rowsrc_make row_chunk_offsets load_row_chunks", 0, (Q + 3) / 4 + Q, c_row_chunks<Q, 1>) \
  X("row_chunks<" #Q ",2>", "rowsrc_make row_chunk_offsets load_row_chunks", 0, (Q + 3) / 4 + Q, c_row_chunks<Q, 2>)
#define LC_PACK_Q(X, Q) \
  X("pack_q<" #Q ">", "packsrc_make dcp_make_rsrc load_pack_q", 2, Q, c_pack_q<Q>)
#define LC_COLS(X, Q) \
  X("cols<" #Q ">", "load_cols", 1, Q, c_cols<Q>) \
  X("nodes<" #Q ">", "store_nodes_q", Q, 0, c_nodes<Q>)
#define LC_LDS(X, N) X("lds<" #N ">", "load_lds_q", 1, N, c_lds<N>)

#define LANE_CASES(X) \
  X("elem_f", "lmin lmin3 llt leq lsel lneg lf_splat lf_pin", 3, 12, c_elem_f) \
  X("elem_u", "llt_u lequ lselu lminu lmaxu lane_shr lu_splat lane_ids land lor lnot", 3, 12, c_elem_u) \
  X("shift_up", "lane_shift_up lane_shift_up_again", 2, 5, c_shift_up) \
  X("shift_keep", "lane_shift_up_keep", 3, 3, c_shift_keep) \
  LC_WAVE_MIN(X, 0, "valu") LC_WAVE_MIN(X, 1, "load") LC_WAVE_MIN(X, 2, "twice") \
  LC_GROUPS(X, 4) LC_GROUPS(X, 8) LC_GROUPS(X, 16) LC_GROUPS(X, 32) \
  X("votes", "wave_any wave_ballot read_lane read_laneu", 4, 6, c_votes) \
  X("lane_policy", "lane leader ballot max_of", 0, 3, c_lane_policy) \
  LC_EXCHANGE(X, 1) LC_MULTI(X, 2) LC_MULTI(X, 4) LC_MULTI(X, 8) \
  X("group1_keep", "get_shift_keep init", 3, 3, c_group1_keep) \
  LC_TDD(X, 3, 2) LC_TDD(X, 6, 2) LC_TDD(X, 4, 4) LC_TDD(X, 6, 4) LC_TDD(X, 8, 4) LC_TDD(X, 4, 8) LC_TDD(X, 8, 8) \
  LC_TDD_STRIP(X, 4, 2) LC_TDD_STRIP(X, 3, 8) LC_TDD_STRIP(X, 4, 8) \
  LC_Q_ALL(X, LC_STASH) LC_Q_ALL(X, LC_LOAD_STORE) \
  LC_CHUNKS(X, 5) LC_CHUNKS(X, 6) LC_CHUNKS(X, 7) LC_CHUNKS(X, 8) LC_CHUNKS(X, 10) \
  LC_PACK_Q(X, 1) LC_PACK_Q(X, 2) LC_PACK_Q(X, 3) LC_PACK_Q(X, 4) LC_PACK_Q(X, 6) LC_PACK_Q(X, 8) \
  X("code_row", "packsrc_make dcp_make_rsrc load_code_row", 2, 5, c_code_row) \
  LC_COLS(X, 1) LC_COLS(X, 2) LC_COLS(X, 3) LC_COLS(X, 4) \
  LC_LDS(X, 1) LC_LDS(X, 2) LC_LDS(X, 4) \
  X("lane_mem", "load_lane store_lane load_f32_at load_u32_at store_f32_where store_sp_lane0 store_u32_lane0 store_f32_lane0", \
    10, 3, c_lane_mem)
