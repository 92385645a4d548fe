// mcmc::Learner::Triangles / WriteTriangles against the statement of include/ammsb_triangles.h over the pi the existing
// accessor fetches (GetPiRow) and the training links: node a is a member of community k iff pi[a, k] >= threshold in
// binary32; a triangle at a is a pair b < c of neighbours of a that are neighbours of each other, and it lies inside every
// community the three share.  The statement marks the neighbours of a in a table and walks every pair the slow way.
// Integers on both sides: every output is equal, and the float64 values, one formula over equal integers, are bit-equal.
//   triangles_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                          DIR/cpp.ckpt, DIR/triangles.txt (threshold 0.05) and DIR/links.txt (the link-communities file,
//                          which lists the training links) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_triangles.h"
#include "postfit_test.h"
typedef mcmc::Learner::TrianglesResult Result;

// the statement over a list of keys -> a result whose Derive() has run
static Result Statement(const std::vector<mcmc::Float>& pi, uint64_t N, uint64_t K, float thr, const std::vector<mcmc::Edge>& keys) {
  std::vector<char> M(N * K);
  for (uint64_t i = 0; i < N * K; ++i) M[i] = pi[i] >= thr;
  std::vector<std::vector<uint32_t>> rows(N);
  Result w;
  uint64_t valid = 0;
  for (mcmc::Edge e : keys) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    if (a >= N || b >= N) {
      ++w.skipped;
      continue;
    }
    ++valid;
    if (a == b) continue;
    rows[a].push_back(static_cast<uint32_t>(b));
    rows[b].push_back(static_cast<uint32_t>(a));
  }
  for (auto& row : rows) {
    std::sort(row.begin(), row.end());
    row.erase(std::unique(row.begin(), row.end()), row.end());
    w.M += row.size();
  }
  w.dropped = valid - w.M / 2;
  w.degree.assign(N, 0);
  w.tri.assign(N, 0);
  w.tri_in.assign(N, 0);
  w.tri_comms.assign(N, 0);
  w.ktri3.assign(K, 0);
  w.kpart.assign(K, 0);
  w.kmembers.assign(K, 0);
  w.wedges.assign(K, 0);
  std::vector<uint64_t> tk(K), c(K);
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<uint32_t>& ra = rows[a];
    w.degree[a] = static_cast<uint32_t>(ra.size());
    std::fill(tk.begin(), tk.end(), 0);
    std::fill(c.begin(), c.end(), 0);
    for (uint32_t b : ra)
      for (uint64_t k = 0; k < K; ++k) c[k] += M[b * K + k];
    for (size_t i = 0; i < ra.size(); ++i)
      for (size_t j = i + 1; j < ra.size(); ++j) {
        const uint64_t b = ra[i], cc = ra[j];
        if (!std::binary_search(rows[b].begin(), rows[b].end(), static_cast<uint32_t>(cc))) continue;
        ++w.tri[a];
        bool in = false;
        for (uint64_t k = 0; k < K; ++k)
          if (M[a * K + k] && M[b * K + k] && M[cc * K + k]) {
            ++tk[k];
            in = true;
          }
        w.tri_in[a] += in;
      }
    for (uint64_t k = 0; k < K; ++k) {
      w.ktri3[k] += tk[k];
      w.kpart[k] += tk[k] > 0;
      w.tri_comms[a] += tk[k] > 0;
      if (M[a * K + k]) {
        ++w.kmembers[k];
        w.wedges[k] += c[k] * (c[k] - 1) / 2;  // (c = 0: 0)
      }
    }
  }
  w.Derive();
  return w;
}

static void Compare(const Result& got, const Result& want) {
  EXPECT(got.degree == want.degree && got.tri == want.tri && got.tri_in == want.tri_in && got.tri_comms == want.tri_comms);
  EXPECT(got.ktri3 == want.ktri3 && got.kpart == want.kpart && got.kmembers == want.kmembers && got.wedges == want.wedges);
  EXPECT(got.M == want.M && got.skipped == want.skipped && got.dropped == want.dropped && got.total == want.total);
  EXPECT(got.triangles == want.triangles);
  EXPECT(SameBits(got.tpr, want.tpr) && SameBits(got.clustering, want.clustering) &&
         SameBits(got.local_clustering, want.local_clustering) && SameBits(got.inside, want.inside));
  EXPECT(memcmp(&got.transitivity, &want.transitivity, sizeof(double)) == 0 &&
         memcmp(&got.avg_clustering, &want.avg_clustering, sizeof(double)) == 0);
}

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  const uint64_t N = cfg.N, K = cfg.K;
  const std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  Result got;
  learner.Triangles(thr, nullptr, &got);
  Compare(got, Statement(pi, N, K, thr, links));
  const uint64_t all = got.total;
  EXPECT(got.skipped == 0 && got.dropped == 0 && got.M == 2 * links.size() && got.total > 0);
  // a list of its own: a loop, a repeat in the other order of the ends, and keys with an end >= N
  std::vector<mcmc::Edge> own;
  for (size_t i = 0; i < links.size(); i += 2) own.push_back(links[i]);
  own.push_back((7ull << 32) | 7ull);
  own.push_back(((own[3] & 0xFFFFFFFFull) << 32) | (own[3] >> 32));
  own.push_back(own[5]);
  own.push_back((static_cast<uint64_t>(N) << 32) | 1ull);
  own.push_back((2ull << 32) | 0xFFFFFFFFull);
  learner.Triangles(thr, &own, &got);
  const Result want = Statement(pi, N, K, thr, own);
  Compare(got, want);
  EXPECT(got.skipped == 2 && got.dropped == 3);
  printf("Triangles thr=%g ok: %llu triangles, %llu in the half list\n", static_cast<double>(thr),
         static_cast<unsigned long long>(all), static_cast<unsigned long long>(want.total));
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  Check(learner, cfg, pi, 0.05f);
  Check(learner, cfg, pi, 1.0f / 64);
  Check(learner, cfg, pi, 0.0f);
  ExpectUnperturbed(fit);
  int threw = 0;
  Result r;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.Triangles(bad, nullptr, &r); });
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/triangles.txt");
    EXPECT(learner.WriteTriangles(&f, 0.05f) && f.good());
    WriteTrainingLinks(learner, d);
    WriteCheckpoint(learner, d);
  }
}

int main(int argc, char** argv) {
  // the derived measures on hand-made integers: a triangle 0 1 2 with a tail 3 at node 2, all in one community; node 4 alone
  Result hand;
  hand.degree = {2, 2, 3, 1, 0};
  hand.tri = {1, 1, 1, 0, 0};
  hand.tri_in = {1, 1, 1, 0, 0};
  hand.tri_comms = {1, 1, 1, 0, 0};
  hand.ktri3 = {3, 0};
  hand.kpart = {3, 0};
  hand.kmembers = {4, 0};
  hand.wedges = {5, 0};  // C(2, 2) + C(2, 2) + C(3, 2) + C(1, 2)
  hand.Derive();
  EXPECT(hand.tpr[0] == 0.75 && hand.tpr[1] == -1.0 && hand.clustering[0] == 3.0 / 5.0 && hand.clustering[1] == -1.0);
  EXPECT(hand.triangles[0] == 1 && hand.total == 1 && hand.transitivity == 3.0 / 5.0);
  EXPECT(hand.local_clustering[0] == 1.0 && hand.local_clustering[2] == 1.0 / 3.0 && hand.local_clustering[3] == -1.0);
  EXPECT(hand.inside[0] == 1.0 && hand.inside[3] == -1.0 && hand.avg_clustering == (1.0 + 1.0 + 1.0 / 3.0) / 3.0);
  hand.ktri3[0] = 4;
  int threw = 0;
  try {
    hand.Derive();
  } catch (const std::logic_error&) {
    ++threw;
  }
  EXPECT(threw == 1);

  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
