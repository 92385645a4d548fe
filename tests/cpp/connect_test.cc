// mcmc::Learner::CommunityLinks / LinkedCommunities / WriteLinkedCommunities against the statement of
// include/ammsb_connect.h over the pi the existing accessor fetches (GetPiRow) and the training links: node a is a member
// of community k iff pi[a, k] >= threshold in binary32; directed[k, l] counts the links (a, b) with a in k and b in l,
// links = directed + its transpose; the partners are a stable selection by exact rationals (128-bit cross-multiplication)
// over w = links[k, l] and pairs = d_k d_l - overlap[k, l].  Integer adds and integer compares: everything is equal.
//   connect_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                        DIR/cpp.ckpt, DIR/linked.txt (threshold 0.05, top 4, density) and DIR/links.txt (the
//                        link-communities file, which lists the training links) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ammsb_connect.h"
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

struct Candidate {
  uint64_t w, den;
  uint32_t l, o;
};

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  typedef unsigned __int128 u128;
  const uint64_t N = cfg.N, K = cfg.K;
  // every training link once
  std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  std::sort(links.begin(), links.end());
  links.erase(std::unique(links.begin(), links.end()), links.end());
  std::vector<std::vector<uint32_t>> in(N);
  std::vector<uint64_t> overlap(K * K, 0), directed(K * K, 0), want(K * K, 0);
  for (uint64_t a = 0; a < N; ++a) {
    for (uint64_t k = 0; k < K; ++k)
      if (pi[a * K + k] >= thr) in[a].push_back(static_cast<uint32_t>(k));
    for (uint32_t k : in[a])
      for (uint32_t l : in[a]) ++overlap[k * K + l];
  }
  for (mcmc::Edge e : links)
    for (uint32_t k : in[e >> 32])
      for (uint32_t l : in[e & 0xFFFFFFFFull]) ++directed[k * K + l];
  for (uint64_t k = 0; k < K; ++k)
    for (uint64_t l = 0; l < K; ++l) want[k * K + l] = directed[k * K + l] + directed[l * K + k];
  std::vector<uint64_t> got;
  learner.CommunityLinks(thr, &got);
  EXPECT(got == want);
  std::vector<uint64_t> size, internal, boundary;
  uint64_t uncovered = 0;
  learner.CommunityQuality(thr, &size, &internal, &boundary, &uncovered);
  for (uint64_t k = 0; k < K; ++k) EXPECT(got[k * K + k] == 2 * internal[k] && size[k] == overlap[k * K + k]);
  uint64_t partners = 0;
  for (const char* by : {"links", "density"})
    for (uint32_t top : {1u, 4u, 64u})
      for (uint64_t min_links : {0ull, 3ull}) {
        mcmc::Learner::Linked r, cut;
        learner.LinkedCommunities(thr, top, by, min_links, &r);
        learner.LinkedCommunities(thr, top, by, min_links, &cut, 4096);
        EXPECT(r.partner == cut.partner && r.links == cut.links && r.shared == cut.shared && r.size == size);
        EXPECT(r.internal == internal && r.valid == links.size() && r.skipped == 0);
        const bool density = std::string(by) == "density";
        for (uint64_t k = 0; k < K; ++k) {
          std::vector<Candidate> c;
          for (uint64_t l = 0; l < K; ++l) {
            const uint64_t w = want[k * K + l];
            if (l == k || w < std::max<uint64_t>(1, min_links)) continue;
            const uint64_t pairs = overlap[k * K + k] * overlap[l * K + l] - overlap[k * K + l];
            if (density && pairs == 0) continue;
            c.push_back({w, density ? pairs : 1, static_cast<uint32_t>(l), static_cast<uint32_t>(overlap[k * K + l])});
          }
          std::stable_sort(c.begin(), c.end(), [](const Candidate& x, const Candidate& y) {
            return static_cast<u128>(x.w) * y.den > static_cast<u128>(y.w) * x.den;  // (stable: equal values stay by l)
          });
          for (uint32_t t = 0; t < top; ++t) {
            const bool have = t < c.size();
            EXPECT(r.partner[k * top + t] == (have ? static_cast<int32_t>(c[t].l) : -1));
            EXPECT(r.links[k * top + t] == (have ? c[t].w : 0u));
            EXPECT(r.shared[k * top + t] == (have ? c[t].o : 0u));
            partners += have;
          }
        }
      }
  printf("LinkedCommunities thr=%g: %llu partner slots compared\n", static_cast<double>(thr), (unsigned long long)partners);
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
  std::vector<mcmc::Float> pi;
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
    pi.insert(pi.end(), row.begin(), row.end());
  }
  // an ordinary threshold, the start value's neighbourhood and one above every value (0 would be K^2 updates per link)
  for (float thr : {0.05f, 1.0f / 64, 2.0f}) Check(learner, cfg, pi, thr);
  // the read-out does not perturb the run: the state after 30 more steps equals that of an undisturbed learner
  mcmc::Learner plain(cfg, queue);
  plain.Run(30);
  plain.Run(30);
  learner.Run(30);
  EXPECT(learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
  EXPECT(learner.GetBeta() == plain.GetBeta() && learner.GetPiRow(17) == plain.GetPiRow(17));
  int threw = 0;
  mcmc::Learner::Linked r;
  std::vector<uint64_t> m;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) {
    try {
      learner.LinkedCommunities(bad, 4, "density", 1, &r);
    } catch (const std::invalid_argument&) {
      ++threw;
    }
    try {
      learner.CommunityLinks(bad, &m);
    } catch (const std::invalid_argument&) {
      ++threw;
    }
  }
  EXPECT(threw == 8);
  for (uint32_t top : {0u, 65u}) {
    try {
      learner.LinkedCommunities(0.05f, top, "density", 1, &r);
    } catch (const std::invalid_argument&) {
      ++threw;
    }
  }
  try {
    learner.LinkedCommunities(0.05f, 4, "jaccard", 1, &r);
  } catch (const std::invalid_argument&) {
    ++threw;
  }
  EXPECT(threw == 11);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/linked.txt");
    EXPECT(learner.WriteLinkedCommunities(&f, 0.05f, 4, "density"));
    std::ofstream lf(d + "/links.txt");  // the training links, for the reader of linked.txt
    EXPECT(learner.WriteLinkCommunities(&lf, 1, 0) && lf.good());
    std::ofstream ck(d + "/cpp.ckpt", std::ios::binary);
    EXPECT(learner.Serialize(&ck));
    EXPECT(f.good() && ck.good());
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
