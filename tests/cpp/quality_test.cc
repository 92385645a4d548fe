// mcmc::Learner::CommunityQuality / WriteCommunityQuality against compares over the pi the existing accessor fetches
// (GetPiRow): node a is a member of k iff pi[a, k] >= threshold in binary32; size[k] = the members, internal[k] /
// boundary[k] = the training links with both ends / exactly one end in k, uncovered = the links whose ends share no
// community.  Integer counts: every figure exactly.
//   quality_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                        DIR/cpp.ckpt, DIR/quality.txt (threshold 0.05) and DIR/links.txt (the training links, as
//                        WriteLinkCommunities lists them) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_quality.h"
#include "mcmc/data.h"
#include "mcmc/learner.h"

namespace clcuda = mcmc::clcuda;

static int fails = 0;
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

static bool Prepare(mcmc::Config* cfg, uint64_t N, std::vector<mcmc::Edge> e) {
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

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Edge>& links, float thr) {
  const uint64_t N = cfg.N, K = cfg.K;
  std::vector<char> member(N * K);
  std::vector<uint64_t> want_size(K, 0), want_in(K, 0), want_out(K, 0);
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
    for (uint64_t k = 0; k < K; ++k) want_size[k] += (member[a * K + k] = row[k] >= thr);
  }
  uint64_t want_uncovered = 0;
  for (mcmc::Edge e : links) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    bool any = false;
    for (uint64_t k = 0; k < K; ++k) {
      const bool x = member[a * K + k], y = member[b * K + k];
      want_in[k] += x && y;
      want_out[k] += x != y;
      any = any || (x && y);
    }
    want_uncovered += !any;
  }
  std::vector<uint64_t> size, internal, boundary;
  uint64_t uncovered = ~0ull;
  learner.CommunityQuality(thr, &size, &internal, &boundary, &uncovered);
  EXPECT(size == want_size);
  EXPECT(internal == want_in);
  EXPECT(boundary == want_out);
  EXPECT(uncovered == want_uncovered);
  uint64_t in = 0, out = 0;
  for (uint64_t k = 0; k < K; ++k) in += internal[k], out += boundary[k];
  printf("CommunityQuality thr=%g over %zu links: internal %llu, boundary %llu, uncovered %llu\n", static_cast<double>(thr),
         links.size(), (unsigned long long)in, (unsigned long long)out, (unsigned long long)uncovered);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  mcmc::Config cfg;
  cfg.device_sampling = cfg.async_launch = cfg.graph_launch = device;
  EXPECT(Prepare(&cfg, N, graph));
  clcuda::Platform platform((size_t)0);
  clcuda::Device dev(platform, 0);
  clcuda::Context context(dev);
  clcuda::Queue queue(context, dev);
  mcmc::Learner learner(cfg, queue);
  learner.Run(30);
  std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  std::sort(links.begin(), links.end());
  links.erase(std::unique(links.begin(), links.end()), links.end());
  // an ordinary threshold, 0 (everybody is a member of everything) and one above every value (all links uncovered)
  for (float thr : {0.05f, 0.0f, 1.0f / 64, 2.0f}) Check(learner, cfg, links, thr);
  std::vector<uint64_t> size, internal, boundary;
  uint64_t uncovered = 0;
  learner.CommunityQuality(0.0f, &size, &internal, &boundary, &uncovered);
  EXPECT(uncovered == 0 && internal == std::vector<uint64_t>(cfg.K, links.size()) && size == std::vector<uint64_t>(cfg.K, N));
  learner.CommunityQuality(2.0f, &size, &internal, &boundary, &uncovered);
  EXPECT(uncovered == links.size() && boundary == std::vector<uint64_t>(cfg.K, 0));
  // the read-out does not perturb the run: the state after 30 more steps equals that of an undisturbed learner
  mcmc::Learner plain(cfg, queue);
  plain.Run(30);
  plain.Run(30);
  learner.Run(30);
  EXPECT(learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
  EXPECT(learner.GetBeta() == plain.GetBeta() && learner.GetPiRow(17) == plain.GetPiRow(17));
  int threw = 0;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) {
    try {
      learner.CommunityQuality(bad, &size, &internal, &boundary, &uncovered);
    } catch (const std::invalid_argument&) {
      ++threw;
    }
  }
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/quality.txt");
    EXPECT(learner.WriteCommunityQuality(&f, 0.05f));
    std::ofstream ck(d + "/cpp.ckpt", std::ios::binary);
    EXPECT(learner.Serialize(&ck));
    std::ofstream lf(d + "/links.txt");
    EXPECT(learner.WriteLinkCommunities(&lf, 1, 0));
    EXPECT(f.good() && ck.good() && lf.good());
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = mcmc::GenerateSyntheticGraph(N, 16, 16, 7);
  EXPECT(edges.size() > 100000);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
  return fails ? 1 : 0;
}
