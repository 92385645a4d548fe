// mcmc::Learner::NodeRoles / WriteNodeRoles against the statement of include/ammsb_roles.h over the pi the existing
// accessor fetches (GetPiRow) and the training adjacency: node a is a member of community k iff pi[a, k] >= threshold in
// binary32, c[a, k] counts the valid targets of row a that are in k, and everything else is sums, compares and a ranking
// of those integers.  Integers on both sides: every output is equal, and the float64 values, one formula over equal
// integers, are bit-equal.
//   roles_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes DIR/cpp.ckpt,
//                      DIR/roles.txt (threshold 0.05, top 4, all) and DIR/links.txt (the link-communities file, which lists
//                      the training links) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_roles.h"
#include "postfit_test.h"
typedef mcmc::Learner::NodeRolesResult Result;

// the statement over a CSR -> a result whose Derive() has run
static Result Statement(const std::vector<mcmc::Float>& pi, uint64_t N, uint64_t K, float thr,
                        const std::vector<uint64_t>& offsets, const std::vector<mcmc::Vertex>& targets, uint32_t top, bool own_only,
                        uint32_t min_count) {
  std::vector<char> M(N * K);
  for (uint64_t i = 0; i < N * K; ++i) M[i] = pi[i] >= thr;
  Result w;
  w.top = top;
  w.degree.assign(N, 0);
  w.own.assign(N, 0);
  w.embedded.assign(N, 0);
  w.reached.assign(N, 0);
  w.hflags.assign(N, 0);
  w.votes.assign(N, 0);
  w.squares.assign(N, 0);
  w.home.assign(N * top, -1);
  w.hcount.assign(N * top, 0);
  w.ksum.assign(K, 0);
  w.ksq.assign(K, 0);
  w.kmembers.assign(K, 0);
  std::vector<uint64_t> c(K);
  std::vector<uint32_t> cand;
  for (uint64_t a = 0; a < N; ++a) {
    std::fill(c.begin(), c.end(), 0);
    for (uint64_t p = offsets[a]; p < offsets[a + 1]; ++p) {
      const uint64_t b = targets[p];
      if (b >= N) {
        ++w.skipped;
        continue;
      }
      ++w.valid;
      ++w.degree[a];
      bool shared = false;
      for (uint64_t k = 0; k < K; ++k) {
        c[k] += M[b * K + k];
        shared = shared || (M[b * K + k] && M[a * K + k]);
      }
      w.embedded[a] += shared;
    }
    cand.clear();
    for (uint64_t k = 0; k < K; ++k) {
      const bool mine = M[a * K + k];
      w.own[a] += mine;
      w.reached[a] += c[k] > 0;
      w.votes[a] += c[k];
      w.squares[a] += c[k] * c[k];
      if (mine) {
        w.ksum[k] += c[k];
        w.ksq[k] += c[k] * c[k];
        ++w.kmembers[k];
      }
      if (own_only ? (mine && c[k] >= min_count) : (c[k] >= std::max<uint64_t>(1, min_count))) cand.push_back(static_cast<uint32_t>(k));
    }
    std::stable_sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) { return c[x] > c[y]; });
    for (uint32_t j = 0; j < top && j < cand.size(); ++j) {
      w.home[a * top + j] = static_cast<int32_t>(cand[j]);
      w.hcount[a * top + j] = static_cast<uint32_t>(c[cand[j]]);
      if (M[a * K + cand[j]]) w.hflags[a] |= 1u << j;
    }
  }
  w.Derive();
  return w;
}

static void Compare(const Result& got, const Result& want) {
  EXPECT(got.degree == want.degree && got.own == want.own && got.embedded == want.embedded && got.reached == want.reached);
  EXPECT(got.votes == want.votes && got.squares == want.squares);
  EXPECT(got.home == want.home && got.hcount == want.hcount && got.hflags == want.hflags);
  EXPECT(got.ksum == want.ksum && got.ksq == want.ksq && got.kmembers == want.kmembers);
  EXPECT(got.valid == want.valid && got.skipped == want.skipped);
  EXPECT(SameBits(got.embeddedness, want.embeddedness) && SameBits(got.participation, want.participation) && SameBits(got.z, want.z));
}

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr, uint32_t top,
                  const std::string& among, uint32_t min_count) {
  const uint64_t N = cfg.N, K = cfg.K;
  std::vector<uint64_t> offsets;
  std::vector<mcmc::Vertex> targets;
  cfg.trainingGraph->ExportCSR(&offsets, &targets);
  Result got;
  learner.NodeRoles(thr, nullptr, top, among, min_count, &got);
  Compare(got, Statement(pi, N, K, thr, offsets, targets, top, among == "own", min_count));
  EXPECT(got.skipped == 0 && got.valid == offsets[N] - offsets[0]);
  // a list of its own: a loop, a repeat, and keys with an end >= N; each valid key sits in both ends' rows
  std::vector<mcmc::Edge> own;
  const std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  for (size_t i = 0; i < links.size(); i += 5) own.push_back(links[i]);
  own.push_back((7ull << 32) | 7ull);
  own.push_back(own[3]);
  own.push_back((static_cast<uint64_t>(N) << 32) | 1ull);
  own.push_back((2ull << 32) | 0xFFFFFFFFull);
  std::vector<std::vector<mcmc::Vertex>> rows(N);
  for (mcmc::Edge e : own) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    if (a >= N || b >= N) continue;
    rows[a].push_back(static_cast<mcmc::Vertex>(b));
    rows[b].push_back(static_cast<mcmc::Vertex>(a));
  }
  offsets.assign(1, 0);
  targets.clear();
  for (uint64_t a = 0; a < N; ++a) {
    targets.insert(targets.end(), rows[a].begin(), rows[a].end());
    offsets.push_back(targets.size());
  }
  learner.NodeRoles(thr, &own, top, among, min_count, &got);
  Result want = Statement(pi, N, K, thr, offsets, targets, top, among == "own", min_count);
  want.skipped = 2;
  Compare(got, want);
  EXPECT(got.degree[7] >= 2);
  printf("NodeRoles thr=%g top=%u %s min_count=%u ok\n", static_cast<double>(thr), top, among.c_str(), min_count);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  Check(learner, cfg, pi, 0.05f, 4, "all", 0);
  Check(learner, cfg, pi, 1.0f / 64, 16, "own", 0);
  Check(learner, cfg, pi, 0.0f, 1, "all", 3);
  Check(learner, cfg, pi, 2.0f, 4, "own", 3);
  ExpectUnperturbed(fit);
  int threw = 0;
  Result r;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.NodeRoles(bad, nullptr, 4, "all", 0, &r); });
  for (uint32_t bad : {0u, 17u}) threw += Throws([&] { learner.NodeRoles(0.05f, nullptr, bad, "all", 0, &r); });
  threw += Throws([&] { learner.NodeRoles(0.05f, nullptr, 4, "some", 0, &r); });
  EXPECT(threw == 7);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/roles.txt");
    EXPECT(learner.WriteNodeRoles(&f, 0.05f) && f.good());
    WriteTrainingLinks(learner, d);
    WriteCheckpoint(learner, d);
  }
}

int main(int argc, char** argv) {
  // the derived measures on hand-made integers: a star of 4 leaves in one community, seen from the centre and a leaf
  Result hand;
  hand.top = 1;
  hand.degree = {4, 1, 0};
  hand.embedded = {4, 1, 0};
  hand.votes = {4, 1, 0};
  hand.squares = {16, 1, 0};
  hand.home = {0, 0, -1};
  hand.hcount = {4, 1, 0};
  hand.hflags = {1, 1, 0};
  hand.own = hand.reached = {1, 1, 0};
  hand.ksum = {8};    // the centre's 4 and four leaves' 1
  hand.ksq = {20};
  hand.kmembers = {5};
  hand.Derive();
  EXPECT(hand.embeddedness[0] == 1.0 && hand.embeddedness[2] == -1.0 && hand.participation[0] == 0.0 && hand.participation[2] == -1.0);
  EXPECT(hand.z[0] == (4.0 - 8.0 / 5.0) / std::sqrt(20.0 / 5.0 - (8.0 / 5.0) * (8.0 / 5.0)) && hand.z[2] == 0.0);

  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
