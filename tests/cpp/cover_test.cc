// mcmc::Learner::CompareCover / WriteCoverMatch against compares over the pi the existing accessor fetches (GetPiRow):
// node a is a member of detected community k iff pi[a, k] >= threshold in binary32; overlap[g, k] = the valid members
// of ground-truth community g that are members of k; the best match maximises overlap / (t_g + d_k), compared by
// integer cross-multiplication, equal rationals to the lower index, none with overlap > 0 -> -1.  Integers: every
// figure exactly.  The ground truth is the cover the generator plants (GenerateSyntheticCover), spoilt with a member
// == N, a member == 2^32 - 1, a duplicate and an empty community.
//   cover_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                      DIR/cpp.ckpt, DIR/match.txt (threshold 0.05) and DIR/truth.txt (the cover, one line per community
//                      `n id0 id1 ...`) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_cover.h"
#include "postfit_test.h"

// o1 / s1 > o2 / s2 (all below 2^32: the products fit 64 bits)
static bool Better(uint64_t o1, uint64_t s1, uint64_t o2, uint64_t s2) { return o1 * s2 > o2 * s1; }

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi,
                  const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, float thr) {
  const uint64_t N = cfg.N, K = cfg.K, G = offsets.size() - 1;
  std::vector<char> member(N * K);
  std::vector<uint64_t> d(K, 0), t(G, 0), ov(G * K, 0);
  for (uint64_t i = 0; i < N * K; ++i) d[i % K] += (member[i] = pi[i] >= thr);
  uint64_t want_skipped = 0;
  for (uint64_t g = 0; g < G; ++g)
    for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) {
      const uint64_t a = members[i];
      if (a >= N) {
        ++want_skipped;
        continue;
      }
      ++t[g];
      for (uint64_t k = 0; k < K; ++k) ov[g * K + k] += member[a * K + k];
    }
  std::vector<int32_t> want_tb(G, -1), want_db(K, -1);
  std::vector<uint32_t> want_to(G, 0), want_do(K, 0);
  for (uint64_t g = 0; g < G; ++g)
    for (uint64_t k = 0; k < K; ++k) {
      const uint64_t o = ov[g * K + k], s = t[g] + d[k];
      if (o == 0) continue;
      if (want_tb[g] < 0 || Better(o, s, want_to[g], t[g] + d[want_tb[g]])) want_tb[g] = k, want_to[g] = o;
      if (want_db[k] < 0 || Better(o, s, want_do[k], t[want_db[k]] + d[k])) want_db[k] = g, want_do[k] = o;
    }
  mcmc::Learner::CoverMatch m, m2;
  std::vector<uint32_t> dense;
  learner.CompareCover(offsets, members, thr, &m, &dense);
  learner.CompareCover(offsets, members, thr, &m2);
  EXPECT(m.detected_size == d);
  EXPECT(m.truth_best == want_tb);
  EXPECT(m.truth_overlap == want_to);
  EXPECT(m.truth_size == std::vector<uint32_t>(t.begin(), t.end()));
  EXPECT(m.detected_best == want_db);
  EXPECT(m.detected_overlap == want_do);
  EXPECT(m.skipped == want_skipped);
  EXPECT(dense == std::vector<uint32_t>(ov.begin(), ov.end()));
  EXPECT(m2.truth_best == m.truth_best && m2.truth_overlap == m.truth_overlap && m2.truth_size == m.truth_size &&
         m2.detected_best == m.detected_best && m2.detected_overlap == m.detected_overlap && m2.skipped == m.skipped);
  // the derived measures, from the formulas of include/ammsb_cover.h
  double sum = 0;
  uint64_t present = 0;
  for (uint64_t g = 0; g < G; ++g) {
    const double f1 = want_tb[g] >= 0 ? 2.0 * want_to[g] / static_cast<double>(t[g] + d[want_tb[g]]) : 0.0;
    EXPECT(m.f1_truth_each[g] == f1);
    if (t[g]) sum += f1, ++present;
  }
  EXPECT(m.f1_truth == (present ? sum / present : -1.0));
  EXPECT(m.avg_f1 == (m.f1_truth >= 0 && m.f1_detected >= 0 ? (m.f1_truth + m.f1_detected) / 2 : -1.0));
  printf("CompareCover thr=%g: G %llu, skipped %llu, f1_truth %.6f, f1_detected %.6f, avg_f1 %.6f\n",
         static_cast<double>(thr), (unsigned long long)G, (unsigned long long)m.skipped, m.f1_truth, m.f1_detected, m.avg_f1);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, const std::vector<uint64_t>& offsets,
                    const std::vector<uint32_t>& members, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  // an ordinary threshold, 0 (everybody is a member of everything), the start value's neighbourhood and one above
  // every value (everything unmatched)
  const std::vector<mcmc::Float> pi = fit.Pi();
  for (float thr : {0.05f, 0.0f, 1.0f / 64, 2.0f}) Check(learner, cfg, pi, offsets, members, thr);
  mcmc::Learner::CoverMatch m;
  learner.CompareCover(offsets, members, 2.0f, &m);
  EXPECT(m.truth_best == std::vector<int32_t>(offsets.size() - 1, -1) && m.detected_best == std::vector<int32_t>(cfg.K, -1));
  EXPECT(m.f1_truth == 0.0 && m.f1_detected == -1.0 && m.avg_f1 == -1.0);
  // nothing to compare: no community, and communities without members
  learner.CompareCover({0}, {}, 0.05f, &m);
  EXPECT(m.truth_best.empty() && m.detected_best == std::vector<int32_t>(cfg.K, -1) && m.f1_truth == -1.0);
  learner.CompareCover({0, 0, 0}, {}, 0.05f, &m);
  EXPECT(m.truth_best == std::vector<int32_t>(2, -1) && m.truth_size == std::vector<uint32_t>(2, 0) && m.f1_truth == -1.0);
  ExpectUnperturbed(fit);
  int threw = 0;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.CompareCover(offsets, members, bad, &m); });
  EXPECT(threw == 4);
  const std::vector<std::vector<uint64_t>> bad_offsets = {{}, {1, 2}, {0, 3, 2, static_cast<uint64_t>(members.size())}, {0, 5}};
  for (const auto& bad : bad_offsets) threw += Throws([&] { learner.CompareCover(bad, members, 0.05f, &m); });
  EXPECT(threw == 8);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/match.txt");
    EXPECT(learner.WriteCoverMatch(&f, offsets, members, 0.05f) && f.good());
    WriteCheckpoint(learner, d);
    WriteTruth(d, offsets, members);
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  std::vector<std::vector<mcmc::Vertex>> cover = PlantedCover(N);
  // every edge of the graph has both ends in a community of the cover
  {
    std::vector<uint32_t> bits(N, 0);
    for (size_t k = 0; k < cover.size(); ++k)
      for (mcmc::Vertex v : cover[k]) bits[v] |= 1u << k;
    size_t outside = 0;
    for (mcmc::Edge e : edges) outside += !(bits[e >> 32] & bits[e & 0xFFFFFFFFull]);
    EXPECT(outside == 0);
  }
  cover[7][3] = cover[7][2];  // this test's own spoiling: a node twice inside a community
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> members;
  SpoiltCover(cover, N, &offsets, &members);
  RunOnce(N, edges, offsets, members, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, offsets, members, true, nullptr);
  return Finish();
}
