// mcmc::Learner::CommunityOverlap / RelatedCommunities / WriteRelatedCommunities against the statement of
// include/ammsb_relate.h over the pi the existing accessor fetches (GetPiRow): node a is a member of community k iff
// pi[a, k] >= threshold in binary32; overlap[k, l] counts the nodes in both; the partners are a stable selection by exact
// rationals (128-bit cross-multiplication).  Integer adds and integer compares: everything is equal, and nothing depends
// on max_bytes.
//   relate_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                       DIR/cpp.ckpt and DIR/related.txt (threshold 0.05, top 4, jaccard) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_relate.h"
#include "postfit_test.h"

struct Candidate {
  uint32_t o, l;
  uint64_t den;
};

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  typedef unsigned __int128 u128;
  const uint64_t N = cfg.N, K = cfg.K;
  std::vector<uint32_t> want(K * K, 0);
  std::vector<uint32_t> in;
  for (uint64_t a = 0; a < N; ++a) {
    in.clear();
    for (uint64_t k = 0; k < K; ++k)
      if (pi[a * K + k] >= thr) in.push_back(static_cast<uint32_t>(k));
    for (uint32_t k : in)
      for (uint32_t l : in) ++want[k * K + l];
  }
  std::vector<uint32_t> got, small;
  learner.CommunityOverlap(thr, &got);
  learner.CommunityOverlap(thr, &small, 1);  // slabs of 64 rows
  EXPECT(got == want && small == want);
  std::vector<uint64_t> sizes;
  learner.Memberships(1, thr, nullptr, nullptr, nullptr, &sizes);
  for (uint64_t k = 0; k < K; ++k) EXPECT(sizes[k] == got[k * K + k]);
  uint64_t partners = 0;
  for (const char* by : {"overlap", "jaccard", "contained"})
    for (uint32_t top : {1u, 4u, 64u})
      for (uint32_t min_overlap : {0u, 3u}) {
        mcmc::Learner::Related r, cut;
        learner.RelatedCommunities(thr, top, by, min_overlap, &r);
        learner.RelatedCommunities(thr, top, by, min_overlap, &cut, 4096);
        EXPECT(r.partner == cut.partner && r.overlap == cut.overlap && r.size == cut.size && r.size == sizes);
        const std::string m(by);
        for (uint64_t k = 0; k < K; ++k) {
          std::vector<Candidate> c;
          for (uint64_t l = 0; l < K; ++l) {
            const uint32_t o = want[k * K + l];
            if (l == k || o < std::max(1u, min_overlap)) continue;
            const uint64_t dk = want[k * K + k], dl = want[l * K + l];
            c.push_back({o, static_cast<uint32_t>(l), m == "overlap" ? 1 : m == "jaccard" ? dk + dl - o : dl});
          }
          std::stable_sort(c.begin(), c.end(), [](const Candidate& x, const Candidate& y) {
            return static_cast<u128>(x.o) * y.den > static_cast<u128>(y.o) * x.den;  // (stable: equal values stay by l)
          });
          for (uint32_t t = 0; t < top; ++t) {
            const bool have = t < c.size();
            EXPECT(r.partner[k * top + t] == (have ? static_cast<int32_t>(c[t].l) : -1));
            EXPECT(r.overlap[k * top + t] == (have ? c[t].o : 0u));
            partners += have;
          }
        }
      }
  printf("RelatedCommunities thr=%g: %llu partner slots compared\n", static_cast<double>(thr), (unsigned long long)partners);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  // an ordinary threshold, 0 (every node in every community), the start value's neighbourhood and one above every value
  for (float thr : {0.05f, 0.0f, 1.0f / 64, 2.0f}) Check(learner, cfg, pi, thr);
  ExpectUnperturbed(fit);
  int threw = 0;
  mcmc::Learner::Related r;
  std::vector<uint32_t> ov;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) {
    threw += Throws([&] { learner.RelatedCommunities(bad, 4, "jaccard", 1, &r); });
    threw += Throws([&] { learner.CommunityOverlap(bad, &ov); });
  }
  EXPECT(threw == 8);
  for (uint32_t top : {0u, 65u}) threw += Throws([&] { learner.RelatedCommunities(0.05f, top, "jaccard", 1, &r); });
  threw += Throws([&] { learner.RelatedCommunities(0.05f, 4, "cosine", 1, &r); });
  EXPECT(threw == 11);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/related.txt");
    EXPECT(learner.WriteRelatedCommunities(&f, 0.05f, 4, "jaccard") && f.good());
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
