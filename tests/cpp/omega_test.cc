// mcmc::Learner::CoverOmega / WriteCoverOmega against the statement of include/ammsb_omega.h over the pi the existing
// accessor fetches (GetPiRow): node a is a member of detected community k iff pi[a, k] >= threshold in binary32; per pair
// of the universe the communities shared in each cover, counted with integer adds: every count is equal.  The results do
// not depend on launch_pairs, bit for bit.
//   omega_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                      DIR/cpp.ckpt, DIR/omega.txt (threshold 0.05, the covered universe) and DIR/truth.txt (the cover,
//                      one line per community `n id0 id1 ...`) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_omega.h"
#include "postfit_test.h"

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi,
                  const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members,
                  const std::vector<uint32_t>& universe, float thr) {
  const uint64_t N = cfg.N, K = cfg.K, G = offsets.size() - 1, n = universe.size();
  std::vector<int64_t> position(N, -1);
  for (uint64_t i = 0; i < n; ++i) position[universe[i]] = static_cast<int64_t>(i);
  std::vector<std::vector<char>> D(n, std::vector<char>(K, 0)), T(n, std::vector<char>(G, 0));
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t k = 0; k < K; ++k) D[i][k] = pi[universe[i] * K + k] >= thr;
  uint64_t skipped = 0, outside = 0;
  for (uint64_t g = 0; g < G; ++g)
    for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) {
      if (members[i] >= N) ++skipped;
      else if (position[members[i]] < 0) ++outside;
      else T[position[members[i]]][g] = 1;
    }
  uint64_t L = 1;
  for (uint64_t i = 0; i < n; ++i)
    L = std::max<uint64_t>(L, 1 + std::max(std::count(D[i].begin(), D[i].end(), 1), std::count(T[i].begin(), T[i].end(), 1)));
  std::vector<uint64_t> agree(L, 0), detected(L, 0), truth(L, 0);
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t j = i + 1; j < n; ++j) {
      uint64_t sD = 0, sT = 0;
      for (uint64_t k = 0; k < K; ++k) sD += D[i][k] & D[j][k];
      for (uint64_t g = 0; g < G; ++g) sT += T[i][g] & T[j][g];
      ++detected[sD];
      ++truth[sT];
      if (sD == sT) ++agree[sD];
    }
  mcmc::Learner::OmegaIndex r, tiles, ragged;
  learner.CoverOmega(offsets, members, thr, universe, &r);
  learner.CoverOmega(offsets, members, thr, universe, &tiles, 1);  // a tile per launch
  learner.CoverOmega(offsets, members, thr, universe, &ragged, 5 * AMMSB_OMEGA_TILE * AMMSB_OMEGA_TILE);
  EXPECT(r.nodes == n && r.skipped == skipped && r.outside == outside);
  EXPECT(r.agree == agree && r.detected == detected && r.truth == truth);
  for (const mcmc::Learner::OmegaIndex* other : {&tiles, &ragged}) {
    EXPECT(r.agree == other->agree && r.detected == other->detected && r.truth == other->truth);
    EXPECT(r.skipped == other->skipped && r.outside == other->outside);
    EXPECT((r.omega == other->omega || (r.omega != r.omega && other->omega != other->omega)));
  }
  // the score is the header's formula over the histograms the call returned
  mcmc::Learner::OmegaIndex want = r;
  want.omega = want.omega_unadjusted = 7;
  want.Derive();
  EXPECT((want.omega == r.omega || (want.omega != want.omega && r.omega != r.omega)));
  EXPECT((want.omega_unadjusted == r.omega_unadjusted || n < 2));
  EXPECT(r.omega != r.omega || r.omega <= 1.0);
  printf("CoverOmega thr=%g: n %llu, L %llu, skipped %llu, outside %llu, omega %.6f\n", static_cast<double>(thr),
         (unsigned long long)n, (unsigned long long)L, (unsigned long long)skipped, (unsigned long long)outside, r.omega);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, const std::vector<uint64_t>& offsets,
                    const std::vector<uint32_t>& members, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  // a ragged universe of 700 nodes (five tile rows and a tail), which leaves some members outside
  std::vector<uint32_t> some;
  for (uint32_t a = 3; some.size() < 700; a += 1 + a % 5) some.push_back(a);
  // an ordinary threshold, 0 (every node in every community), the start value's neighbourhood and one above every value
  for (float thr : {0.05f, 0.0f, 1.0f / 64, 2.0f}) Check(learner, cfg, pi, offsets, members, some, thr);
  const std::vector<uint32_t> covered = mcmc::Learner::OmegaUniverse("covered", members, N);
  EXPECT(std::is_sorted(covered.begin(), covered.end()) && !covered.empty() && covered.back() < N);
  EXPECT(mcmc::Learner::OmegaUniverse("all", members, N).size() == N);
  mcmc::Learner::OmegaIndex r;
  learner.CoverOmega(offsets, members, 0.05f, {}, &r);  // nothing to pair
  EXPECT(r.nodes == 0 && r.omega != r.omega && r.agree == std::vector<uint64_t>(1, 0));
  EXPECT(r.skipped == 2 && r.outside == members.size() - 2);  // the members are counted without a universe too
  {  // a ground truth in another id space: every member is >= N, "covered" is empty, and all of them are skipped
    const std::vector<uint64_t> woff = {0, 3, 3, 5};
    const std::vector<uint32_t> wmem = {static_cast<uint32_t>(N), static_cast<uint32_t>(N + 7), 0xFFFFFFFFu,
                                        static_cast<uint32_t>(N + 1), static_cast<uint32_t>(2 * N)};
    const std::vector<uint32_t> none = mcmc::Learner::OmegaUniverse("covered", wmem, N);
    EXPECT(none.empty());
    learner.CoverOmega(woff, wmem, 0.05f, none, &r);
    EXPECT(r.nodes == 0 && r.skipped == 5 && r.outside == 0 && r.omega != r.omega && r.agree == std::vector<uint64_t>(1, 0));
    learner.CoverOmega(woff, wmem, 0.05f, some, &r);  // the same counts from the device
    EXPECT(r.nodes == 700 && r.skipped == 5 && r.outside == 0 && r.truth[0] == 700ull * 699 / 2);
  }
  learner.CoverOmega(offsets, members, 0.05f, {5}, &r);
  EXPECT(r.nodes == 1 && r.omega != r.omega);
  learner.CoverOmega({0}, {}, 2.0f, some, &r);  // all pairs at level 0 in both covers
  EXPECT(r.omega != r.omega && r.omega_unadjusted == 1.0 && r.agree[0] == 700ull * 699 / 2);
  ExpectUnperturbed(fit);
  int threw = 0;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.CoverOmega(offsets, members, bad, some, &r); });
  EXPECT(threw == 4);
  const std::vector<std::vector<uint32_t>> bad_universes = {{5, 4}, {4, 4}, {1, static_cast<uint32_t>(N)}};
  for (const auto& bad : bad_universes) threw += Throws([&] { learner.CoverOmega(offsets, members, 0.05f, bad, &r); });
  EXPECT(threw == 7);
  std::vector<uint32_t> twice = members;
  twice[offsets[7] + 3] = twice[offsets[7] + 2];
  threw += Throws([&] { learner.CoverOmega(offsets, twice, 0.05f, some, &r); });
  threw += Throws([&] { mcmc::Learner::OmegaUniverse("some", members, N); });
  EXPECT(threw == 9);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/omega.txt");
    EXPECT(learner.WriteCoverOmega(&f, offsets, members, 0.05f, covered) && f.good());
    WriteCheckpoint(learner, d);
    WriteTruth(d, offsets, members);
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  // the planted cover of the first 2000 nodes only: the covered universe is a small share of the nodes
  std::vector<std::vector<mcmc::Vertex>> cover = PlantedCover(N);
  for (auto& c : cover) c.erase(std::remove_if(c.begin(), c.end(), [](mcmc::Vertex a) { return a >= 2000; }), c.end());
  // a member == N, a member == 2^32 - 1, an empty community and a small one; no node twice inside a community
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> members;
  SpoiltCover(cover, N, &offsets, &members);
  RunOnce(N, edges, offsets, members, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, offsets, members, true, nullptr);
  return Finish();
}
