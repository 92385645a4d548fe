// What the C++ callers of mcmc::Learner's post-fit API (tests/cpp/<analysis>_test.cc) have in common, once: the EXPECT
// macro and its counter, the data set and the fitted learner every one of them starts from (N nodes of the synthetic
// graph, K = 64, 30 steps), the "reading does not perturb the run" check, the count of refused arguments, the files
// the other hosts read (cpp.ckpt, links.txt, truth.txt) and the last line.  A test keeps what is its own -- its
// statement, its thresholds, its bad arguments -- and its main() stays a short list of what it does:
//   const std::vector<mcmc::Edge> edges = TestGraph(N);
//   RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);   // Fitted fit(N, edges, device); ...; ExpectUnperturbed(fit);
//   RunOnce(N, edges, true, nullptr);
//   return Finish();
// Header-only, one include per program; everything is inline, so a test that does not use a piece pays nothing for it.
#ifndef AMMSB_TESTS_CPP_POSTFIT_TEST_H_
#define AMMSB_TESTS_CPP_POSTFIT_TEST_H_

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "mcmc/data.h"
#include "mcmc/learner.h"

namespace clcuda = mcmc::clcuda;

inline int fails = 0;
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

// the last line of every program -> its exit status
inline int Finish() {
  printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
  return fails ? 1 : 0;
}

inline bool Prepare(mcmc::Config* cfg, uint64_t N, std::vector<mcmc::Edge> e) {
  cfg->N = N;
  cfg->K = 64;
  cfg->mini_batch_size = 256;
  cfg->num_node_sample = 16;
  cfg->heldout_ratio = 0.05;
  cfg->alpha = static_cast<mcmc::Float>(1) / cfg->K;
  cfg->phi_wg_size = cfg->beta_wg_size = cfg->ppx_wg_size = 64;
  cfg->beta_seed = {44, 45};
  cfg->neighbor_seed = {56, 57};
  srand(12345);
  bool ok = false;
  for (int attempt = 0; attempt < 64 && !ok; ++attempt) {
    cfg->training_edges.clear();
    cfg->heldout_edges.clear();
    ok = mcmc::GenerateSetsFromEdges(cfg->N, e, cfg->heldout_ratio, &cfg->training_edges, &cfg->heldout_edges,
                                     &cfg->training, &cfg->heldout);
    if (!ok) e.resize(e.size() - 40);
  }
  if (!ok) return false;
  cfg->trainingGraph.reset(new mcmc::Graph(cfg->N, cfg->training_edges));
  cfg->heldoutGraph.reset(new mcmc::Graph(cfg->N, cfg->heldout_edges));
  cfg->E = e.size();
  return true;
}

// the graph every program runs on
inline std::vector<mcmc::Edge> TestGraph(uint64_t N) {
  std::vector<mcmc::Edge> edges = mcmc::GenerateSyntheticGraph(N, 16, 16, 7);
  EXPECT(edges.size() > 100000);
  return edges;
}

// The config of one run: host sampling and the synchronous loop, or device sampling + async + graph launch.  A base of
// Fitted, so that the data set is drawn (rand()) before the first device call, as every test has always done.
struct PreparedConfig {
  mcmc::Config cfg;
  PreparedConfig(uint64_t N, const std::vector<mcmc::Edge>& edges, bool device) {
    cfg.device_sampling = cfg.async_launch = cfg.graph_launch = device;
    EXPECT(Prepare(&cfg, N, edges));
  }
};

// ... and the learner over it after 30 steps.  The learner refers to cfg: a Fitted stays where it was made.
struct Fitted : PreparedConfig {
  clcuda::Platform platform;
  clcuda::Device dev;
  clcuda::Context context;
  clcuda::Queue queue;
  mcmc::Learner learner;

  Fitted(uint64_t N, const std::vector<mcmc::Edge>& edges, bool device)
      : PreparedConfig(N, edges, device), platform((size_t)0), dev(platform, 0), context(dev), queue(context, dev), learner(cfg, queue) {
    learner.Run(30);
  }
  Fitted(const Fitted&) = delete;

  // all of pi, [N, K], through the accessor that was there before the post-fit API: one GetPiRow per node
  std::vector<mcmc::Float> Pi() {
    std::vector<mcmc::Float> pi;
    for (uint64_t a = 0; a < cfg.N; ++a) {
      const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
      pi.insert(pi.end(), row.begin(), row.end());
    }
    return pi;
  }
};

// what was read out did not perturb the run: the state after 30 more steps equals that of an undisturbed learner
inline void ExpectUnperturbed(Fitted& fit) {
  mcmc::Learner plain(fit.cfg, fit.queue);
  plain.Run(30);
  plain.Run(30);
  fit.learner.Run(30);
  EXPECT(fit.learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
  EXPECT(fit.learner.GetBeta() == plain.GetBeta() && fit.learner.GetPiRow(17) == plain.GetPiRow(17));
}

// did the call refuse its arguments?  std::invalid_argument and nothing wider: any other exception ends the program
template <class Call>
inline bool Throws(Call call) {
  try {
    call();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// every training link once, ascending
inline std::vector<mcmc::Edge> SortedTrainingLinks(const mcmc::Config& cfg) {
  std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  std::sort(links.begin(), links.end());
  links.erase(std::unique(links.begin(), links.end()), links.end());
  return links;
}

inline void WriteCheckpoint(mcmc::Learner& learner, const std::string& dir) {
  std::ofstream ck(dir + "/cpp.ckpt", std::ios::binary);
  EXPECT(learner.Serialize(&ck));
  EXPECT(ck.good());
}

// the link-communities file, which lists the training links: for the reader of a file of figures over them
inline void WriteTrainingLinks(mcmc::Learner& learner, const std::string& dir) {
  std::ofstream lf(dir + "/links.txt");
  EXPECT(learner.WriteLinkCommunities(&lf, 1, 0) && lf.good());
}

// The ground truth of cover_test, nmi_test and omega_test: the cover the generator plants ...
inline std::vector<std::vector<mcmc::Vertex>> PlantedCover(uint64_t N) {
  std::vector<std::vector<mcmc::Vertex>> cover = mcmc::GenerateSyntheticCover(N, 16, 7);
  EXPECT(cover.size() == 16);
  return cover;
}

// ... spoilt with a member == N, a member == 2^32 - 1, an empty community at position 9 and a small last one, as
// community g = members[offsets[g] .. offsets[g + 1]) ...
inline void SpoiltCover(std::vector<std::vector<mcmc::Vertex>> cover, uint64_t N, std::vector<uint64_t>* offsets,
                        std::vector<uint32_t>* members) {
  cover[2][1] = static_cast<mcmc::Vertex>(N);
  cover[5].back() = 0xFFFFFFFFu;
  cover.insert(cover.begin() + 9, std::vector<mcmc::Vertex>());
  cover.push_back({3, 1, 4});
  offsets->assign(1, 0);
  members->clear();
  for (const auto& c : cover) {
    members->insert(members->end(), c.begin(), c.end());
    offsets->push_back(members->size());
  }
}

// ... and as a file, one line `n id0 id1 ...` per community
inline void WriteTruth(const std::string& dir, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members) {
  std::ofstream tf(dir + "/truth.txt");
  for (size_t g = 0; g + 1 < offsets.size(); ++g) {
    tf << offsets[g + 1] - offsets[g];
    for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) tf << " " << members[i];
    tf << "\n";
  }
  EXPECT(tf.good());
}

inline uint32_t Bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

template <class T>
inline bool SameBits(const std::vector<T>& x, const std::vector<T>& y) {
  return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0);
}

#endif  // AMMSB_TESTS_CPP_POSTFIT_TEST_H_
