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
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_quality.h"
#include "postfit_test.h"

static void Check(Fitted& fit, const std::vector<mcmc::Edge>& links, float thr) {
  const uint64_t N = fit.cfg.N, K = fit.cfg.K;
  std::vector<char> member(N * K);
  std::vector<uint64_t> want_size(K, 0), want_in(K, 0), want_out(K, 0);
  const std::vector<mcmc::Float> pi = fit.Pi();  // (fetched for every threshold)
  for (uint64_t i = 0; i < N * K; ++i) want_size[i % K] += (member[i] = pi[i] >= thr);
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
  fit.learner.CommunityQuality(thr, &size, &internal, &boundary, &uncovered);
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
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Edge> links = SortedTrainingLinks(cfg);
  // an ordinary threshold, 0 (everybody is a member of everything) and one above every value (all links uncovered)
  for (float thr : {0.05f, 0.0f, 1.0f / 64, 2.0f}) Check(fit, links, thr);
  std::vector<uint64_t> size, internal, boundary;
  uint64_t uncovered = 0;
  learner.CommunityQuality(0.0f, &size, &internal, &boundary, &uncovered);
  EXPECT(uncovered == 0 && internal == std::vector<uint64_t>(cfg.K, links.size()) && size == std::vector<uint64_t>(cfg.K, N));
  learner.CommunityQuality(2.0f, &size, &internal, &boundary, &uncovered);
  EXPECT(uncovered == links.size() && boundary == std::vector<uint64_t>(cfg.K, 0));
  ExpectUnperturbed(fit);
  int threw = 0;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY})
    threw += Throws([&] { learner.CommunityQuality(bad, &size, &internal, &boundary, &uncovered); });
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/quality.txt");
    EXPECT(learner.WriteCommunityQuality(&f, 0.05f) && f.good());
    WriteCheckpoint(learner, d);
    WriteTrainingLinks(learner, d);
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
