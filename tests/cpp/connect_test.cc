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
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_connect.h"
#include "postfit_test.h"

struct Candidate {
  uint64_t w, den;
  uint32_t l, o;
};

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  typedef unsigned __int128 u128;
  const uint64_t N = cfg.N, K = cfg.K;
  const std::vector<mcmc::Edge> links = SortedTrainingLinks(cfg);
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
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  // an ordinary threshold, the start value's neighbourhood and one above every value (0 would be K^2 updates per link)
  for (float thr : {0.05f, 1.0f / 64, 2.0f}) Check(learner, cfg, pi, thr);
  ExpectUnperturbed(fit);
  int threw = 0;
  mcmc::Learner::Linked r;
  std::vector<uint64_t> m;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) {
    threw += Throws([&] { learner.LinkedCommunities(bad, 4, "density", 1, &r); });
    threw += Throws([&] { learner.CommunityLinks(bad, &m); });
  }
  EXPECT(threw == 8);
  for (uint32_t top : {0u, 65u}) threw += Throws([&] { learner.LinkedCommunities(0.05f, top, "density", 1, &r); });
  threw += Throws([&] { learner.LinkedCommunities(0.05f, 4, "jaccard", 1, &r); });
  EXPECT(threw == 11);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/linked.txt");
    EXPECT(learner.WriteLinkedCommunities(&f, 0.05f, 4, "density") && f.good());
    WriteTrainingLinks(learner, d);
    WriteCheckpoint(learner, d);
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
