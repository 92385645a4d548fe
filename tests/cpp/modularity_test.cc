// mcmc::Learner::Modularity / WriteModularity against the statement of include/ammsb_modularity.h over the pi the existing
// accessor fetches (GetPiRow) and the training links: node a is a member of community k iff pi[a, k] >= threshold in
// binary32, O_a counts its communities, IN[k] adds floor(2^62 / (O_a O_b)) per link inside k and SV[k] adds deg[a] floor(2^62
// / O_a) per member, both in unsigned 128 bits.  Integer adds on both sides: the sums are equal, and the float64 values,
// one formula over equal integers, are bit-equal.
//   modularity_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                           DIR/cpp.ckpt, DIR/modularity.txt (threshold 0.05) and DIR/links.txt (the link-communities
//                           file, which lists the training links) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "ammsb_modularity.h"
#include "postfit_test.h"
typedef unsigned __int128 u128;

// the statement over a list of keys -> a score whose Derive() has run
static mcmc::Learner::ModularityScore Statement(const std::vector<mcmc::Float>& pi, uint64_t N, uint64_t K, float thr,
                                                const std::vector<mcmc::Edge>& keys) {
  const u128 F = static_cast<u128>(1) << AMMSB_MODULARITY_FRAC_BITS;
  std::vector<std::vector<uint32_t>> in(N);
  for (uint64_t a = 0; a < N; ++a)
    for (uint64_t k = 0; k < K; ++k)
      if (pi[a * K + k] >= thr) in[a].push_back(static_cast<uint32_t>(k));
  mcmc::Learner::ModularityScore want;
  want.internal.assign(K, 0);
  want.volume.assign(K, 0);
  want.degree.assign(N, 0);
  for (mcmc::Edge e : keys) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    if (a >= N || b >= N) {
      ++want.skipped;
      continue;
    }
    ++want.links;
    ++want.degree[a];
    ++want.degree[b];
    if (in[a].empty() || in[b].empty()) continue;
    const u128 w = F / (static_cast<u128>(in[a].size()) * in[b].size());
    std::vector<uint32_t> both;
    std::set_intersection(in[a].begin(), in[a].end(), in[b].begin(), in[b].end(), std::back_inserter(both));
    for (uint32_t k : both) want.internal[k] += w;
  }
  for (uint64_t a = 0; a < N; ++a)
    for (uint32_t k : in[a]) want.volume[k] += static_cast<u128>(want.degree[a]) * (F / in[a].size());
  want.Derive();
  return want;
}

static void Compare(const mcmc::Learner::ModularityScore& got, const mcmc::Learner::ModularityScore& want) {
  EXPECT(got.internal == want.internal && got.volume == want.volume && got.degree == want.degree);
  EXPECT(got.links == want.links && got.skipped == want.skipped);
  EXPECT(SameBits(got.q_each, want.q_each) && SameBits(got.in_each, want.in_each) && SameBits(got.s_each, want.s_each));
  EXPECT(memcmp(&got.q, &want.q, sizeof(double)) == 0);
}

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  const uint64_t N = cfg.N, K = cfg.K;
  const std::vector<mcmc::Edge> links = SortedTrainingLinks(cfg);
  mcmc::Learner::ModularityScore got;
  learner.Modularity(thr, nullptr, &got);
  const mcmc::Learner::ModularityScore want = Statement(pi, N, K, thr, links);
  Compare(got, want);
  EXPECT(got.skipped == 0 && got.links == links.size());
  // a list of its own: the ends the other way round, a loop, a repeat and keys with an end >= N
  std::vector<mcmc::Edge> own;
  for (size_t i = 0; i < links.size(); i += 5) own.push_back((links[i] << 32) | (links[i] >> 32));
  own.push_back((7ull << 32) | 7ull);
  own.push_back(own[3]);
  own.push_back((static_cast<uint64_t>(N) << 32) | 1ull);
  own.push_back((2ull << 32) | 0xFFFFFFFFull);
  learner.Modularity(thr, &own, &got);
  Compare(got, Statement(pi, N, K, thr, own));
  EXPECT(got.skipped == 2);
  printf("Modularity thr=%g: q = %.17g over %llu links\n", static_cast<double>(thr), want.q, (unsigned long long)want.links);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  // an ordinary threshold, the start value's neighbourhood, every stored number (O = K everywhere) and one above every value
  for (float thr : {0.05f, 1.0f / 64, 0.0f, 2.0f}) Check(learner, cfg, pi, thr);
  ExpectUnperturbed(fit);
  int threw = 0;
  mcmc::Learner::ModularityScore r;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.Modularity(bad, nullptr, &r); });
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/modularity.txt");
    EXPECT(learner.WriteModularity(&f, 0.05f) && f.good());
    WriteTrainingLinks(learner, d);
    WriteCheckpoint(learner, d);
  }
}

int main(int argc, char** argv) {
  // the derived measures on hand-made integers: one community that holds both nodes of one link, q = 0 exactly
  mcmc::Learner::ModularityScore hand;
  hand.internal = {static_cast<u128>(1) << 62};
  hand.volume = {static_cast<u128>(2) << 62};
  hand.links = 1;
  hand.Derive();
  EXPECT(hand.q == 0.0 && hand.in_each[0] == 1.0 && hand.s_each[0] == 2.0);
  hand.links = 0;
  hand.Derive();
  EXPECT(hand.q == -1.0 && hand.q_each[0] == -1.0);

  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
