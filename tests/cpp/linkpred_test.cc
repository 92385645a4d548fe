// mcmc::Learner::LinkProbabilities / PredictLinks against arithmetic over the pi and beta the existing accessors fetch
// (GetPiRow, GetBeta): p64 = eps + sum_k pi_ak pi_bk (beta_k - eps) in double over the stored binary32 values, under
// |got - p64| <= (K + 8) 2^-24 M + 2^-100 with M = eps + sum_k pi_ak pi_bk |beta_k - eps| (derived: at most K + 3
// roundings touch a term).  PredictLinks with the tie-tolerant check: every returned score is within the bound of its
// id's p64, no returned id is ineligible, and no eligible node left out has a p64 above the worst returned p64 by more
// than twice the bound.
//   linkpred_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                         DIR/cpp.ckpt and DIR/links.txt (200 nodes, top 10, exclude all) of the first run, for an
//                         exact check from the other host.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_linkpred.h"
#include "postfit_test.h"

struct Model {
  uint64_t N, K;
  std::vector<double> pi, w, aw;  // [N, K], beta_k - eps, |beta_k - eps|
  double eps;
  void P(uint64_t a, uint64_t b, double* p, double* bound) const {
    double s = 0, m = 0;
    for (uint64_t k = 0; k < K; ++k) {
      const double t = pi[a * K + k] * pi[b * K + k];
      s += t * w[k];
      m += t * aw[k];
    }
    *p = eps + s;
    *bound = (K + 8) * std::ldexp(1.0, -24) * (eps + m) + std::ldexp(1.0, -100);
  }
};

static Model Fetch(Fitted& fit) {
  Model m;
  m.N = fit.cfg.N;
  m.K = fit.cfg.K;
  m.eps = static_cast<double>(mcmc::MakeKernelParams(fit.cfg).epsilon);
  const std::vector<mcmc::Float> pi = fit.Pi();
  m.pi.assign(pi.begin(), pi.end());
  const std::vector<mcmc::Float> beta = fit.learner.GetBeta();
  for (uint64_t k = 0; k < m.K; ++k) {
    m.w.push_back(static_cast<double>(beta[2 * k + 1]) - m.eps);
    m.aw.push_back(std::fabs(m.w.back()));
  }
  return m;
}

static mcmc::Edge Key(uint64_t a, uint64_t b) { return (std::min(a, b) << 32) | std::max(a, b); }

static void CheckPairs(mcmc::Learner& learner, const mcmc::Config& cfg, const Model& m) {
  std::vector<mcmc::Edge> edges(cfg.heldout_edges.begin(), cfg.heldout_edges.end());
  const size_t held = edges.size();
  for (size_t i = 0; i < 500 && i < held; ++i) edges.push_back((edges[i] << 32) | (edges[i] >> 32));  // ends swapped
  edges.push_back((7ull << 32) | 7ull);                                                                // a == b
  edges.push_back((static_cast<uint64_t>(m.N) << 32) | 3ull);                                          // out of range
  std::vector<mcmc::Float> got;
  learner.LinkProbabilities(edges, &got);
  EXPECT(got.size() == edges.size());
  uint64_t bad = 0;
  double worst = 0;
  for (size_t i = 0; i + 1 < edges.size(); ++i) {
    double p, bound;
    m.P(edges[i] >> 32, edges[i] & 0xFFFFFFFFull, &p, &bound);
    const double err = std::fabs(static_cast<double>(got[i]) - p);
    worst = std::max(worst, err / bound);
    bad += !(err <= bound);
  }
  EXPECT(bad == 0);
  EXPECT(got.back() == -1.0f);
  printf("LinkProbabilities: %zu pairs, worst error / bound %.3f, past the bound %llu\n", edges.size(), worst,
         (unsigned long long)bad);
}

static void CheckTop(mcmc::Learner& learner, const mcmc::Config& cfg, const Model& m, const std::vector<mcmc::Vertex>& nodes,
                     uint32_t top, uint32_t mask) {
  std::vector<mcmc::Vertex> ids;
  std::vector<mcmc::Float> scores;
  learner.PredictLinks(nodes, top, mask, &ids, &scores);
  EXPECT(ids.size() == nodes.size() * top && scores.size() == ids.size());
  uint64_t bad = 0, heldout_hits = 0;
  std::vector<char> returned(m.N);
  for (size_t i = 0; i < nodes.size(); ++i) {
    const uint64_t a = nodes[i];
    std::fill(returned.begin(), returned.end(), 0);
    double worst_p = 1e300, max_bound = 0;
    uint32_t n = 0;
    for (uint32_t t = 0; t < top; ++t) {
      const mcmc::Vertex b = ids[i * top + t];
      if (b == AMMSB_LINKPRED_NONE) {
        bad += scores[i * top + t] != 0;
        continue;
      }
      bad += n != t;  // empty slots only at the end
      ++n;
      bad += b >= m.N || b == a || returned[b];
      if (b >= m.N) continue;
      returned[b] = 1;
      if (mask & mcmc::Learner::kExcludeTraining) bad += cfg.training->Has(Key(a, b));
      if (mask & mcmc::Learner::kExcludeHeldout) bad += cfg.heldout->Has(Key(a, b));
      heldout_hits += cfg.heldout->Has(Key(a, b));
      double p, bound;
      m.P(a, b, &p, &bound);
      bad += !(std::fabs(static_cast<double>(scores[i * top + t]) - p) <= bound);
      if (t > 0 && ids[i * top + t - 1] != AMMSB_LINKPRED_NONE) {
        const float prev = scores[i * top + t - 1], cur = scores[i * top + t];
        bad += !(prev > cur || (prev == cur && ids[i * top + t - 1] < b));
      }
      worst_p = std::min(worst_p, p);
      max_bound = std::max(max_bound, bound);
    }
    uint64_t eligible = 0;
    for (uint64_t b = 0; b < m.N; ++b) {
      if (b == a) continue;
      if ((mask & mcmc::Learner::kExcludeTraining) && cfg.training->Has(Key(a, b))) continue;
      if ((mask & mcmc::Learner::kExcludeHeldout) && cfg.heldout->Has(Key(a, b))) continue;
      ++eligible;
      if (returned[b]) continue;
      double p, bound;
      m.P(a, b, &p, &bound);
      bad += n == top ? !(p <= worst_p + 2 * std::max(bound, max_bound)) : 1;  // a list with room left nobody out
    }
    bad += n != std::min<uint64_t>(top, eligible);
  }
  EXPECT(bad == 0);
  printf("PredictLinks top=%u mask=%u over %zu nodes: mismatches %llu, held-out links returned %llu\n", top, mask,
         nodes.size(), (unsigned long long)bad, (unsigned long long)heldout_hits);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& edges, bool device, const char* dir) {
  Fitted fit(N, edges, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const Model m = Fetch(fit);
  CheckPairs(learner, cfg, m);
  std::vector<mcmc::Vertex> nodes;
  for (uint32_t i = 0; i < 150; ++i) nodes.push_back(static_cast<mcmc::Vertex>((i * 131u) % N));
  nodes.push_back(nodes[3]);  // a repeat
  const uint32_t all = mcmc::Learner::kExcludeTraining | mcmc::Learner::kExcludeHeldout;
  CheckTop(learner, cfg, m, nodes, 10, all);
  CheckTop(learner, cfg, m, nodes, 64, mcmc::Learner::kExcludeTraining);
  CheckTop(learner, cfg, m, std::vector<mcmc::Vertex>(nodes.begin(), nodes.begin() + 7), 1, 0);
  ExpectUnperturbed(fit);
  int threw = 0;
  std::vector<mcmc::Vertex> ids;
  std::vector<mcmc::Float> scores;
  threw += Throws([&] { learner.PredictLinks(nodes, 0, all, &ids, &scores); });
  threw += Throws([&] { learner.PredictLinks(nodes, 65, all, &ids, &scores); });
  threw += Throws([&] { learner.PredictLinks(nodes, 10, 4, &ids, &scores); });
  threw += Throws([&] { learner.PredictLinks({static_cast<mcmc::Vertex>(N)}, 10, all, &ids, &scores); });
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on since Fetch: the file and the checkpoint are of the same, current state)
    std::vector<mcmc::Vertex> q(nodes.begin(), nodes.begin() + 151);
    std::ofstream f(d + "/links.txt");
    EXPECT(learner.WritePredictedLinks(&f, q, 10, all) && f.good());
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
