// hmm_model.cpp -- see hmm_model.h
#include "hmm_model.h"
#include "../../include/deciphon_host.h"
#include "dcp_errors.h"
#include "dcp_types.h"
#include "host_logic.h"
#include "parallel_for.h"
#include "press_batch.h"

#include <ctype.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace
{

char const AMINO[] = "ACDEFGHIKLMNPQRSTVWY"; // imm_amino_iupac symbols, the order of HMMER's 20 columns

// imm_lprob_add: log(e^x + e^y) in float
float lprob_add(float x, float y)
{
  if (x == y) return (float)(x + M_LN2); // -inf + -inf stays -inf
  float const d = x - y;
  return d > 0 ? x + log1pf(expf(-d)) : y + log1pf(expf(d));
}

// model.c: log1_p -- log(1 - p) from log(p)
float log1_p(float logp) { return log1pf(-expf(logp)); }

// ACGT indices of codon i of an NCBI table listed in TCAG order
void tcag_codon(int i, int out[3])
{
  static int const base[4] = {3, 1, 0, 2}; // T C A G -> A C G T indices
  out[0] = base[i / 16];
  out[1] = base[(i / 4) % 4];
  out[2] = base[i % 4];
}

int amino_index(char aa)
{
  char const *p = strchr(AMINO, aa);
  return aa && p ? (int)(p - AMINO) : -1;
}

// whitespace-separated tokens of one line
struct Tokens
{
  std::vector<char const *> at;
  std::vector<size_t> len;
  explicit Tokens(std::string const &s)
  {
    size_t i = 0, n = s.size();
    while (i < n)
    {
      while (i < n && isspace((unsigned char)s[i])) ++i;
      size_t j = i;
      while (j < n && !isspace((unsigned char)s[j])) ++j;
      if (j > i)
      {
        at.push_back(s.data() + i);
        len.push_back(j - i);
      }
      i = j;
    }
  }
  size_t size() const { return at.size(); }
  bool is(size_t i, char const *w) const { return i < size() && len[i] == strlen(w) && !memcmp(at[i], w, len[i]); }
  std::string str(size_t i) const { return std::string(at[i], len[i]); }
};

// A HMMER3 value is -log(p): parsed as double, negated, then narrowed to float; "*" is p = 0, i.e. -inf.
bool value(Tokens const &t, size_t i, float &out)
{
  if (i >= t.size()) return false;
  if (t.len[i] == 1 && t.at[i][0] == '*')
  {
    out = -INFINITY;
    return true;
  }
  std::string const s = t.str(i);
  char *end = nullptr;
  double const x = strtod(s.c_str(), &end);
  if (end != s.c_str() + s.size() || !isfinite(x)) return false;
  out = (float)-x;
  return true;
}

bool values(Tokens const &t, size_t first, int n, float *out)
{
  if (t.size() < first + (size_t)n) return false;
  for (int i = 0; i < n; ++i)
    if (!value(t, first + (size_t)i, out[i])) return false;
  return true;
}

} // namespace

bool dcp_setup_nuclt_dist(int gencode_id, float const lodds[20], DcpNucltDist &out)
{
  // the translation table, codon i of NCBI's TCAG order
  char aa[64];
  int codon[64][3];
  uint8_t probe[3];
  for (int i = 0; i < 64; ++i)
  {
    tcag_codon(i, codon[i]);
    for (int j = 0; j < 3; ++j) probe[j] = (uint8_t)codon[i][j];
    aa[i] = dcp_gencode_amino(gencode_id, probe);
    if (!aa[i]) return false;
  }
  // codon_lprob (c-core/model.c:361-395): amino log-odds shared by its synonymous codons, stops left at -inf
  int count[20] = {};
  for (int i = 0; i < 64; ++i)
    if (amino_index(aa[i]) >= 0) ++count[amino_index(aa[i])];
  float per_codon[20];
  for (int i = 0; i < 20; ++i) per_codon[i] = lodds[i] - logf((float)count[i]);
  float codonp[64]; // a * 16 + b * 4 + c
  for (int i = 0; i < 64; ++i) codonp[i] = -INFINITY;
  for (int i = 0; i < 64; ++i)
    if (amino_index(aa[i]) >= 0) codonp[codon[i][0] * 16 + codon[i][1] * 4 + codon[i][2]] = per_codon[amino_index(aa[i])];
  // imm_codon_lprob_normalize
  float norm = -INFINITY;
  for (int i = 0; i < 64; ++i) norm = lprob_add(norm, codonp[i]);
  for (int i = 0; i < 64; ++i) codonp[i] -= norm;
  // nuclt_lprob (c-core/model.c:341-359): every base of every codon, a third of the codon's probability
  float const third = logf(3);
  for (int j = 0; j < 4; ++j) out.nucltp[j] = -INFINITY;
  for (int i = 0; i < 64; ++i)
  {
    if (amino_index(aa[i]) < 0) continue;
    float const lp = codonp[codon[i][0] * 16 + codon[i][1] * 4 + codon[i][2]];
    for (int j = 0; j < 3; ++j) out.nucltp[codon[i][j]] = lprob_add(out.nucltp[codon[i][j]], lp - third);
  }
  // imm_codon_marg: index 4 of a position sums over its four bases
  for (int a = 0; a < 5; ++a)
    for (int b = 0; b < 5; ++b)
      for (int c = 0; c < 5; ++c)
      {
        float v = -INFINITY;
        for (int x = 0; x < 4; ++x)
          for (int y = 0; y < 4; ++y)
            for (int z = 0; z < 4; ++z)
              if ((a == 4 || a == x) && (b == 4 || b == y) && (c == 4 || c == z)) v = lprob_add(v, codonp[x * 16 + y * 4 + z]);
        out.codonm[a * 25 + b * 5 + c] = v;
      }
  return true;
}

DcpHmmReader::~DcpHmmReader() { close(); }

void DcpHmmReader::close()
{
  if (fp_) fclose(fp_);
  fp_ = nullptr;
  free(buf_);
  buf_ = nullptr;
  cap_ = 0;
  count_ = 0;
  lengths_.clear();
  end_ = false;
}

bool dcp_setup_models(int gencode_id, float null_lprobs[20], DcpNucltDist &null, DcpNucltDist &bg)
{
  // init_null_lprobs (c-core/hmm_reader.c:76-102): HMMER3's Swiss-Prot 50.8 amino frequencies
  static double const freq[20] = {0.0787945, 0.0151600, 0.0535222, 0.0668298, 0.0397062, 0.0695071, 0.0229198,
                                  0.0590092, 0.0594422, 0.0963728, 0.0237718, 0.0414386, 0.0482904, 0.0395639,
                                  0.0540978, 0.0683364, 0.0540687, 0.0673417, 0.0114135, 0.0304133};
  for (int i = 0; i < 20; ++i) null_lprobs[i] = logf((float)freq[i]);
  float const zero[20] = {};
  return dcp_setup_nuclt_dist(gencode_id, null_lprobs, null) && dcp_setup_nuclt_dist(gencode_id, zero, bg);
}

int DcpHmmReader::open(char const *path, int gencode_id)
{
  close();
  if (!dcp_setup_models(gencode_id, null_lprobs_, null_, bg_)) return DCP_EGENCODEID;
  gencode_ = gencode_id;
  if (!path || !(fp_ = fopen(path, "rb"))) return DCP_EFOPEN;
  // press.c: count_proteins
  while (line())
  {
    if (!line_.compare(0, 8, "HMMER3/f")) ++count_;
    else if (!line_.compare(0, 5, "LENG ")) lengths_.push_back(atol(line_.c_str() + 5));
  }
  if (ferror(fp_))
  {
    close();
    return DCP_EFREAD;
  }
  rewind(fp_);
  return 0;
}

bool DcpHmmReader::line()
{
  ssize_t const n = getline(&buf_, &cap_, fp_);
  if (n < 0) return false;
  line_.assign(buf_, (size_t)n);
  return true;
}

int DcpHmmReader::next(DcpHmmProfile &out)
{
  if (!fp_ || end_) return DCP_EFUNCUSE;
  return profile(out);
}

// hmm_reader_next (c-core/hmm_reader.c:19-67) over one HMMER3/f profile
int DcpHmmReader::profile(DcpHmmProfile &x)
{
  // the profile's first line; blank lines before it are skipped, the end of the file ends the reading
  for (;;)
  {
    if (!line())
    {
      if (ferror(fp_)) return DCP_EFREAD;
      end_ = true;
      return 0;
    }
    Tokens t(line_);
    if (!t.size()) continue;
    if (line_.compare(0, 8, "HMMER3/f")) return DCP_EREADHMMER3;
    break;
  }
  // header: ACC, LENG and GA are what the model keeps; it ends at the HMM line and its transition-name line
  x.accession.clear();
  x.has_ga = false;
  long K = -1;
  for (;;)
  {
    if (!line()) return DCP_EREADHMMER3;
    Tokens t(line_);
    if (!t.size()) continue;
    if (t.is(0, "ACC"))
    {
      if (t.size() < 2) return DCP_EREADHMMER3;
      x.accession = t.str(1);
    }
    else if (t.is(0, "LENG"))
    {
      if (t.size() < 2) return DCP_EREADHMMER3;
      std::string const s = t.str(1);
      char *end = nullptr;
      K = strtol(s.c_str(), &end, 10);
      if (end != s.c_str() + s.size() || K < 0) return DCP_EREADHMMER3;
    }
    else if (t.is(0, "GA"))
      x.has_ga = true;
    else if (t.is(0, "HMM"))
      break;
  }
  if (K < 0) return DCP_EREADHMMER3;
  if (K == 0) return DCP_EZEROMODEL;              // model_setup, c-core/model.c:196
  if (K > DCP_MODEL_MAX) return DCP_ELARGEMODEL;  // c-core/model.c:198
  if (x.accession.size() >= 32) return DCP_ELONGACCESSION; // struct protein accession[32], c-core/protein.c:56-60
  if (!line()) return DCP_EENDOFFILE; // m->m m->i ... names

  int const n = (int)K;
  x.core_size = n;
  x.consensus.assign((size_t)n, ' ');
  std::vector<float> T((size_t)(n + 1) * 7); // T[0]: the transitions that follow COMPO (node 0)
  x.nodes.resize((size_t)n);
  x.lodds.resize((size_t)n * 20);
  float v[20];

  // COMPO (optional; its emissions are not used), the insert emissions of node 0 and its transitions
  if (!line()) return DCP_EENDOFFILE;
  {
    Tokens t(line_);
    if (t.is(0, "COMPO") && !line()) return DCP_EENDOFFILE;
  }
  if (!values(Tokens(line_), 0, 20, v)) return DCP_EREADHMMER3;
  if (!line()) return DCP_EENDOFFILE;
  if (!values(Tokens(line_), 0, 7, T.data())) return DCP_EREADHMMER3;

  // nodes 1..K, then `//`
  int k = 0;
  for (;;)
  {
    if (!line()) return DCP_EENDOFNODES;
    Tokens t(line_);
    if (!t.size()) continue;
    if (t.is(0, "//")) break;
    if (k == n) return DCP_ELARGEMODEL; // model_add_node past core_size, c-core/model.c:63
    // "<k> <20 match values> <MAP> <CONS> ...", then 20 insert values, then 7 transitions
    if (t.str(0) != std::to_string(k + 1) || !values(t, 1, 20, v) || t.size() < 23) return DCP_EENDOFNODES;
    x.consensus[(size_t)k] = t.at[22][0];
    float *lodds = x.lodds.data() + 20 * (size_t)k;
    for (int i = 0; i < 20; ++i) lodds[i] = v[i] - null_lprobs_[i]; // model_add_node, c-core/model.c:67-69
    dcp_setup_nuclt_dist(gencode_, lodds, x.nodes[(size_t)k]);
    if (!line() || !values(Tokens(line_), 0, 20, v)) return DCP_EENDOFNODES;
    if (!line() || !values(Tokens(line_), 0, 7, T.data() + 7 * (size_t)(k + 1))) return DCP_EENDOFNODES;
    ++k;
  }
  if (k != n) return DCP_EENDOFNODES;

  // protein_absorb (c-core/protein.c:98-106): node i carries the transitions out of model node i + 1
  x.trans.resize((size_t)(n + 1) * 7);
  for (int i = 0; i <= n; ++i)
    memcpy(x.trans.data() + 7 * (size_t)i, T.data() + 7 * (size_t)(i + 1 < n ? i + 1 : n), 7 * sizeof(float));

  // calculate_occupancy (c-core/model.c:281-306): MM MI MD IM II DM DD = 0..6
  std::vector<float> locc((size_t)n);
  locc[0] = lprob_add(T[1], T[0]);
  for (int i = 1; i < n; ++i)
  {
    float const *t = T.data() + 7 * (size_t)i;
    float const v0 = locc[(size_t)i - 1] + lprob_add(t[0], t[1]);
    float const v1 = log1_p(locc[(size_t)i - 1]) + t[5];
    locc[(size_t)i] = lprob_add(v0, v1);
  }
  float logZ = -INFINITY;
  for (int i = 0; i < n; ++i) logZ = lprob_add(logZ, locc[(size_t)i] + logf((float)(n - i)));
  for (int i = 0; i < n; ++i) locc[(size_t)i] -= logZ;
  x.BMk.swap(locc);
  return 0;
}

// ---- C ABI: include/deciphon_host.h dcp_hmm_* ----

struct dcp_hmm
{
  DcpHmmReader reader;
  DcpHmmProfile profile;
  bool have = false;
};

extern "C" {

int dcp_hmm_open(char const *path, int gencode_id, struct dcp_hmm **out)
{
  if (!path || !out) return DCP_EFUNCUSE;
  *out = nullptr;
  dcp_hmm *x = new dcp_hmm;
  if (int rc = x->reader.open(path, gencode_id))
  {
    delete x;
    return rc;
  }
  *out = x;
  return 0;
}

void dcp_hmm_close(struct dcp_hmm *x) { delete x; }
long dcp_hmm_count(struct dcp_hmm const *x) { return x ? x->reader.count() : 0; }
int dcp_hmm_end(struct dcp_hmm const *x) { return x ? (int)x->reader.end() : 1; }

int dcp_hmm_next(struct dcp_hmm *x)
{
  if (!x) return DCP_EFUNCUSE;
  x->have = false;
  if (int rc = x->reader.next(x->profile)) return rc;
  x->have = !x->reader.end();
  return 0;
}

int dcp_hmm_core_size(struct dcp_hmm const *x) { return x && x->have ? x->profile.core_size : 0; }
int dcp_hmm_has_ga(struct dcp_hmm const *x) { return x && x->have ? (int)x->profile.has_ga : 0; }

int dcp_hmm_read(struct dcp_hmm const *x, float *trans, float *BMk, float *nucltp, float *codonm, char *accession,
                 char *consensus)
{
  if (!x || !x->have) return DCP_EFUNCUSE;
  DcpHmmProfile const &p = x->profile;
  size_t const K = (size_t)p.core_size;
  if (trans) memcpy(trans, p.trans.data(), p.trans.size() * sizeof(float));
  if (BMk) memcpy(BMk, p.BMk.data(), K * sizeof(float));
  for (size_t e = 0; e < K + 3; ++e)
  {
    DcpNucltDist const &d = e == 0 ? x->reader.null_dist() : e == 1 ? x->reader.bg_dist() : p.nodes[e - 2 < K ? e - 2 : K - 1];
    if (nucltp) memcpy(nucltp + 4 * e, d.nucltp, sizeof d.nucltp);
    if (codonm) memcpy(codonm + 125 * e, d.codonm, sizeof d.codonm);
  }
  if (accession) memcpy(accession, p.accession.c_str(), p.accession.size() + 1);
  if (consensus) memcpy(consensus, p.consensus.c_str(), K + 1);
  return 0;
}

int dcp_hmm_read_lodds(struct dcp_hmm const *x, float *lodds)
{
  if (!x || !x->have || !lodds) return DCP_EFUNCUSE;
  memcpy(lodds, x->profile.lodds.data(), x->profile.lodds.size() * sizeof(float));
  return 0;
}

int dcp_hmm_models(int gencode_id, float *nucltp8, float *codonm250)
{
  float null_lprobs[20];
  DcpNucltDist d[2];
  if (!dcp_setup_models(gencode_id, null_lprobs, d[0], d[1])) return DCP_EGENCODEID;
  for (int e = 0; e < 2; ++e)
  {
    if (nucltp8) memcpy(nucltp8 + 4 * e, d[e].nucltp, sizeof d[e].nucltp);
    if (codonm250) memcpy(codonm250 + 125 * e, d[e].codonm, sizeof d[e].codonm);
  }
  return 0;
}

int dcp_regencode_entries(int gencode_id, int64_t n, float const *lodds, int max_threads, float *entries)
{
  if (n < 0 || (n > 0 && (!lodds || !entries))) return DCP_EFUNCUSE;
  {
    DcpNucltDist probe;
    float const zero[20] = {};
    if (!dcp_setup_nuclt_dist(gencode_id, zero, probe)) return DCP_EGENCODEID;
  }
  unsigned const threads = (unsigned)std::min(std::max(max_threads, 1), 16);
  dcp_parallel_for((size_t)n, threads, 64, 64, [=](size_t i) {
    DcpNucltDist d;
    dcp_setup_nuclt_dist(gencode_id, lodds + 20 * i, d);
    dcp_press_put_entry(entries + i * DCP_PRESS_IN_STRIDE, d);
  });
  return 0;
}

} // extern "C"
