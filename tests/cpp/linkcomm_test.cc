// mcmc::Learner::LinkCommunities / LinkCommunitySizes / WriteLinkCommunities against arithmetic over the pi and beta
// the existing accessors fetch (GetPiRow, GetBeta).  Terms and ids exactly: t_k = (pi_ak * pi_bk) * beta_k in binary32
// (two multiplications, nothing to contract), sorted by (term descending, community ascending) over the terms that are
// > 0 and >= min_term.  prob under |got - p64| <= (K + 8) 2^-24 M + 2^-100, M = eps + sum_k pi_ak pi_bk |beta_k - eps|
// (include/ammsb_linkcomm.h derives it).  Sizes against the count of slot 0 over the training links.
//   linkcomm_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                         DIR/cpp.ckpt and DIR/linkcomm.txt (top 3, min_term 0) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_linkcomm.h"
#include "postfit_test.h"

struct Model {
  uint64_t N, K;
  std::vector<float> pi, beta;  // [N, K], beta_k
  float eps;
};

static Model Fetch(Fitted& fit) {
  Model m;
  m.N = fit.cfg.N;
  m.K = fit.cfg.K;
  m.eps = mcmc::MakeKernelParams(fit.cfg).epsilon;
  m.pi = fit.Pi();
  const std::vector<mcmc::Float> beta = fit.learner.GetBeta();
  for (uint64_t k = 0; k < m.K; ++k) m.beta.push_back(beta[2 * k + 1]);
  return m;
}

// -> mismatching edges; slot0[i] = the community in slot 0 (K: none, K + 1: an end out of range)
static uint64_t Check(mcmc::Learner& learner, const Model& m, const std::vector<mcmc::Edge>& edges, uint32_t top,
                      float min_term, std::vector<uint32_t>* slot0) {
  std::vector<uint32_t> ids;
  std::vector<mcmc::Float> terms, prob;
  learner.LinkCommunities(edges, top, min_term, &ids, &terms, &prob);
  EXPECT(ids.size() == edges.size() * top && terms.size() == ids.size() && prob.size() == edges.size());
  uint64_t bad = 0;
  double worst = 0;
  slot0->assign(edges.size(), 0);
  std::vector<std::pair<uint32_t, uint32_t>> keys;  // (~term bits, k): ascending = term descending, then k ascending
  for (size_t i = 0; i < edges.size(); ++i) {
    const uint64_t a = edges[i] >> 32, b = edges[i] & 0xFFFFFFFFull;
    if (a >= m.N || b >= m.N) {
      bool ok = prob[i] == -1.0f;
      for (uint32_t t = 0; t < top; ++t) ok = ok && ids[i * top + t] == AMMSB_LINKCOMM_NONE && Bits(terms[i * top + t]) == 0;
      bad += !ok;
      (*slot0)[i] = static_cast<uint32_t>(m.K + 1);
      continue;
    }
    keys.clear();
    double s = 0, mag = 0;
    for (uint64_t k = 0; k < m.K; ++k) {
      const volatile float q = m.pi[a * m.K + k] * m.pi[b * m.K + k];
      const volatile float t = q * m.beta[k];
      if (t > 0.0f && t >= min_term) keys.emplace_back(~Bits(t), static_cast<uint32_t>(k));
      const double q64 = static_cast<double>(m.pi[a * m.K + k]) * static_cast<double>(m.pi[b * m.K + k]);
      const double w = static_cast<double>(m.beta[k]) - static_cast<double>(m.eps);
      s += q64 * w;
      mag += q64 * std::fabs(w);
    }
    std::sort(keys.begin(), keys.end());
    bool ok = true;
    for (uint32_t t = 0; t < top; ++t) {
      const uint32_t want_id = t < keys.size() ? keys[t].second : AMMSB_LINKCOMM_NONE;
      const uint32_t want_bits = t < keys.size() ? ~keys[t].first : 0u;
      ok = ok && ids[i * top + t] == want_id && Bits(terms[i * top + t]) == want_bits;
    }
    (*slot0)[i] = keys.empty() ? static_cast<uint32_t>(m.K) : keys[0].second;
    const double bound = (m.K + 8) * std::ldexp(1.0, -24) * (m.eps + mag) + std::ldexp(1.0, -100);
    const double err = std::fabs(static_cast<double>(prob[i]) - (m.eps + s));
    worst = std::max(worst, err / bound);
    bad += !(ok && err <= bound);
  }
  printf("LinkCommunities top=%u min_term=%g over %zu edges: mismatches %llu, worst prob error / bound %.3f\n", top,
         static_cast<double>(min_term), edges.size(), (unsigned long long)bad, worst);
  return bad;
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const Model m = Fetch(fit);
  const std::vector<mcmc::Edge> links = SortedTrainingLinks(fit.cfg);
  std::vector<mcmc::Edge> edges(links.begin(), links.begin() + std::min<size_t>(links.size(), 20000));
  for (size_t i = 0; i < 500; ++i) edges.push_back((edges[i] << 32) | (edges[i] >> 32));  // ends swapped
  edges.push_back((7ull << 32) | 7ull);                                                   // a == b
  edges.push_back((static_cast<uint64_t>(N) << 32) | 3ull);                               // out of range
  edges.push_back((3ull << 32) | 0xFFFFFFFFull);
  std::vector<uint32_t> slot0;
  EXPECT(Check(learner, m, edges, 1, 0.0f, &slot0) == 0);
  EXPECT(Check(learner, m, edges, 4, 0.0f, &slot0) == 0);
  EXPECT(Check(learner, m, edges, 16, 1e-3f, &slot0) == 0);
  // the sizes of the training links against slot 0 of the full call, at two floors
  for (float min_term : {0.0f, 1e-3f}) {
    EXPECT(Check(learner, m, links, 1, min_term, &slot0) == 0);
    std::vector<uint64_t> want(m.K + 1, 0), sizes;
    for (uint32_t k : slot0) ++want[k];
    learner.LinkCommunitySizes(min_term, &sizes);
    uint64_t total = 0;
    for (uint64_t c : sizes) total += c;
    EXPECT(sizes == want && total == links.size());
    printf("LinkCommunitySizes min_term=%g: %llu links, %llu unexplained\n", static_cast<double>(min_term),
           (unsigned long long)total, (unsigned long long)sizes[m.K]);
  }
  ExpectUnperturbed(fit);
  int threw = 0;
  std::vector<uint32_t> ids;
  std::vector<mcmc::Float> terms, prob;
  std::vector<uint64_t> sizes;
  threw += Throws([&] { learner.LinkCommunities(edges, 0, 0, &ids, &terms, &prob); });
  threw += Throws([&] { learner.LinkCommunities(edges, 17, 0, &ids, &terms, &prob); });
  threw += Throws([&] { learner.LinkCommunities(edges, 1, -1e-9f, &ids, &terms, &prob); });
  threw += Throws([&] { learner.LinkCommunities(edges, 1, NAN, &ids, &terms, &prob); });
  threw += Throws([&] { learner.LinkCommunitySizes(INFINITY, &sizes); });
  EXPECT(threw == 5);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on since Fetch: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/linkcomm.txt");
    EXPECT(learner.WriteLinkCommunities(&f, 3, 0) && f.good());
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
