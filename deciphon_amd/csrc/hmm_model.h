// hmm_model.h -- the host half of press: a HMMER3 text reader and the protein model built from it.
//
// Replaces, for dcp_press_*, c-core/hmm_reader.c (hmm_reader_next, init_null_lprobs), the third-party hmr
// library it drives (HMMER3/f text, restated from the format: header keys, COMPO, per node 20 match values,
// the annotation columns, 20 insert values and 7 transitions, `//`), c-core/model.c (setup_nuclt_dist,
// codon_lprob, nuclt_lprob, calculate_occupancy, model_add_node / model_add_trans) and the node layout of
// protein_absorb (c-core/protein.c:66-121).  The arithmetic of third-party imm that model.c calls
// (imm_codon_lprob_normalize, imm_codon_marg, imm_lprob_add) is restated in float; tests/test_press_host.py
// pins the result against the reference's own pressed tests/golden/minifam.dcp.
//
// Nothing here touches the GPU: the emission tables are made from nucltp / codonm by the kernel of
// press_kernel.hip.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

// One nucleotide distribution (struct nuclt_dist, c-core/nuclt_dist.h): 4 nucleotide log-probabilities and the
// 5 x 5 x 5 codon marginals (index 4 = any nucleotide), a * 25 + b * 5 + c.
struct DcpNucltDist
{
  float nucltp[4];
  float codonm[125];
};

// One profile as protein_absorb lays it out.
struct DcpHmmProfile
{
  std::string accession;
  std::string consensus; // K residues
  int core_size = 0;
  bool has_ga = false;
  std::vector<float> trans;        // [(K+1) * 7] MM MI MD IM II DM DD: node i holds T[min(i + 1, K)]
  std::vector<float> BMk;          // [K] occupancy entry (entry_dist = 2)
  std::vector<DcpNucltDist> nodes; // [K] match distribution of node n; node K repeats node K - 1
  std::vector<float> lodds;        // [K * 20] the amino log-odds `nodes` were set up from: they hold under every table
};

// Sets up the nucleotide distribution of amino log-odds `lodds[20]` (ACDEFGHIKLMNPQRSTVWY) under NCBI
// translation table `gencode_id` (setup_nuclt_dist, c-core/model.c:397-411).  false: unknown table.
bool dcp_setup_nuclt_dist(int gencode_id, float const lodds[20], DcpNucltDist &out);

// The models every profile of a file shares (init_null_lprobs, c-core/hmm_reader.c:76-102): the log of HMMER3's
// Swiss-Prot amino frequencies, the null model set up from them and the background set up from log-odds 0, under
// table `gencode_id`.  false: unknown table.
bool dcp_setup_models(int gencode_id, float null_lprobs[20], DcpNucltDist &null, DcpNucltDist &bg);

// Reader of a HMMER3 text file, one profile per next().  All return 0 or a DCP_E* code.
class DcpHmmReader
{
public:
  DcpHmmReader() = default;
  ~DcpHmmReader();
  DcpHmmReader(DcpHmmReader const &) = delete;
  DcpHmmReader &operator=(DcpHmmReader const &) = delete;

  // DCP_EGENCODEID for an unknown translation table, DCP_EFOPEN when the file cannot be read.
  int open(char const *path, int gencode_id);
  void close();
  // press.c: count_proteins -- the number of lines that begin with "HMMER3/f", counted at open
  long count() const { return count_; }
  // what the LENG lines announce, in file order, from the same pass at open: what a caller sizes its buffers by
  // before the first profile is parsed (an estimate: next() is what validates a profile)
  std::vector<long> const &announced_lengths() const { return lengths_; }
  // Reads the next profile into `out`.  At the end of the file it returns 0 and end() becomes true.
  int next(DcpHmmProfile &out);
  bool end() const { return end_; }
  // the null model (Swiss-Prot amino frequencies) and the background (log-odds 0): the same for every profile
  DcpNucltDist const &null_dist() const { return null_; }
  DcpNucltDist const &bg_dist() const { return bg_; }

private:
  bool line(); // the next line into line_; false at end of file
  int profile(DcpHmmProfile &out);

  FILE *fp_ = nullptr;
  char *buf_ = nullptr;
  size_t cap_ = 0;
  std::string line_;
  long count_ = 0;
  std::vector<long> lengths_;
  bool end_ = false;
  int gencode_ = 0;
  float null_lprobs_[20] = {};
  DcpNucltDist null_{}, bg_{};
};
