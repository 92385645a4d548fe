// mcmc::Learner::CoverNMI / WriteCoverNMI against the float64 statement of include/ammsb_nmi.h over the pi the existing
// accessor fetches (GetPiRow): node a is a member of detected community k iff pi[a, k] >= threshold in binary32; the
// integers t, d, o from compares; h(x) = -(x / N) log2(x / N) with the host's log2.  Every entropy within 2^-47 S of the
// statement, S the sum of the magnitudes of the h-terms that enter it (for a minimum: the largest S among the
// qualifying pairs, since |min a - min b| <= max |a - b|); +inf exactly, i.e. the fallback taken on both sides.  The
// statement's qualifying inequality must not be borderline (exactly 0 or above 1e-9) for the comparison to mean
// anything: that is checked first.  The results do not depend on the slab size, bit for bit.
//   nmi_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                    DIR/cpp.ckpt, DIR/nmi.txt (threshold 0.05) and DIR/truth.txt (the cover, one line per community
//                    `n id0 id1 ...`) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "ammsb_nmi.h"
#include "postfit_test.h"

static const double kInf = std::numeric_limits<double>::infinity();
static const double kTol = std::ldexp(1.0, -47);

static double H1(int64_t x, double n) {
  if (x == 0) return 0.0;
  const double p = static_cast<double>(x) / n;
  return -(p * std::log2(p));
}

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi,
                  const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, float thr) {
  const int64_t N = cfg.N, K = cfg.K, G = offsets.size() - 1;
  const double n = static_cast<double>(N);
  std::vector<char> member(N * K);
  std::vector<int64_t> d(K, 0), t(G, 0), ov(G * K, 0);
  for (int64_t i = 0; i < N * K; ++i) d[i % K] += (member[i] = pi[i] >= thr);
  uint64_t want_skipped = 0;
  for (int64_t g = 0; g < G; ++g)
    for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) {
      const int64_t a = members[i];
      if (a >= N) {
        ++want_skipped;
        continue;
      }
      ++t[g];
      for (int64_t k = 0; k < K; ++k) ov[g * K + k] += member[a * K + k];
    }
  std::vector<double> HX(G), HY(K), SX(G), SY(K), cX(G, kInf), cY(K, kInf), sX(G, 0), sY(K, 0);
  for (int64_t g = 0; g < G; ++g) HX[g] = t[g] >= N ? 0 : H1(t[g], n) + H1(N - t[g], n), SX[g] = std::fabs(HX[g]) + 1e-300;
  for (int64_t k = 0; k < K; ++k) HY[k] = d[k] >= N ? 0 : H1(d[k], n) + H1(N - d[k], n);
  double gap = kInf;
  for (int64_t g = 0; g < G; ++g)
    for (int64_t k = 0; k < K; ++k) {
      const int64_t o = ov[g * K + k], n10 = t[g] - o, n01 = d[k] - o, n00 = N - t[g] - d[k] + o;
      if (n00 < 0) continue;
      const double a = H1(o, n), b = H1(n00, n), c = H1(n01, n), e = H1(n10, n), lhs = a + b, rhs = c + e;
      if (lhs != rhs) gap = std::min(gap, std::fabs(lhs - rhs));
      if (!(lhs >= rhs)) continue;
      const double J = lhs + rhs, S = std::fabs(a) + std::fabs(b) + std::fabs(c) + std::fabs(e);
      cX[g] = std::min(cX[g], std::max(0.0, J - HY[k]));
      cY[k] = std::min(cY[k], std::max(0.0, J - HX[g]));
      // (H(Y_k) and H(X_g) are sums of two such magnitudes themselves)
      sX[g] = std::max(sX[g], S + std::fabs(HY[k]));
      sY[k] = std::max(sY[k], S + std::fabs(HX[g]));
    }
  EXPECT(gap > 1e-9);  // no borderline pair: the comparison below is meaningful
  mcmc::Learner::CoverNmi r, rows, again;
  learner.CoverNMI(offsets, members, thr, &r);
  learner.CoverNMI(offsets, members, thr, &rows, 1);  // a slab per community
  learner.CoverNMI(offsets, members, thr, &again, 5 * 4 * K);
  EXPECT(r.detected_size == std::vector<uint64_t>(d.begin(), d.end()));
  EXPECT(r.truth_size == std::vector<uint32_t>(t.begin(), t.end()));
  EXPECT(r.skipped == want_skipped);
  for (const mcmc::Learner::CoverNmi* other : {&rows, &again}) {
    EXPECT(SameBits(r.H_truth, other->H_truth) && SameBits(r.h_truth, other->h_truth));
    EXPECT(SameBits(r.H_detected, other->H_detected) && SameBits(r.h_detected, other->h_detected));
    EXPECT(r.nmi_lfk == other->nmi_lfk && r.nmi_max == other->nmi_max && r.skipped == other->skipped);
  }
  mcmc::Learner::CoverNmi want = r;
  for (int64_t g = 0; g < G; ++g) {
    EXPECT(std::fabs(r.H_truth[g] - HX[g]) <= kTol * std::fabs(HX[g]));
    // the fallback is taken on both sides or on neither, where the minimum is not within rounding of the entropy
    const double h = std::min(cX[g], HX[g]);
    EXPECT(std::fabs(r.h_truth[g] - h) <= kTol * std::max(sX[g], std::fabs(HX[g])));
    want.H_truth[g] = r.H_truth[g];
  }
  for (int64_t k = 0; k < K; ++k) {
    EXPECT(std::fabs(r.H_detected[k] - HY[k]) <= kTol * std::fabs(HY[k]));
    const double h = std::min(cY[k], HY[k]);
    EXPECT(std::fabs(r.h_detected[k] - h) <= kTol * std::max(sY[k], std::fabs(HY[k])));
  }
  // the scores are the header's formulas over the arrays the call returned
  want.nmi_lfk = want.nmi_max = 7;
  want.Derive();
  EXPECT(want.nmi_lfk == r.nmi_lfk && want.nmi_max == r.nmi_max);
  EXPECT(r.nmi_lfk == -1.0 || (r.nmi_lfk >= 0 && r.nmi_lfk <= 1));
  printf("CoverNMI thr=%g: G %lld, skipped %llu, nmi_lfk %.6f, nmi_max %.6f, smallest gap %.3g\n", static_cast<double>(thr),
         (long long)G, (unsigned long long)r.skipped, r.nmi_lfk, r.nmi_max, gap);
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, const std::vector<uint64_t>& offsets,
                    const std::vector<uint32_t>& members, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  // an ordinary threshold, 0 (every d_k = N: H(Y_k) = 0), the start value's neighbourhood and one above every value
  for (float thr : {0.05f, 0.0f, 1.0f / 64, 2.0f}) Check(learner, cfg, pi, offsets, members, thr);
  mcmc::Learner::CoverNmi r;
  learner.CoverNMI(offsets, members, 2.0f, &r);  // every detected community is empty: nothing to average on that side
  EXPECT(r.nmi_lfk == -1.0 && r.H_detected == std::vector<double>(cfg.K, 0.0));
  learner.CoverNMI(offsets, members, 0.0f, &r);  // every detected community is everybody: the same
  EXPECT(r.nmi_lfk == -1.0 && r.H_detected == std::vector<double>(cfg.K, 0.0));
  // nothing to compare: no community, and communities without members
  learner.CoverNMI({0}, {}, 0.05f, &r);
  EXPECT(r.H_truth.empty() && r.nmi_lfk == -1.0 && r.H_detected.size() == cfg.K);
  learner.CoverNMI({0, 0, 0}, {}, 0.05f, &r);
  EXPECT(r.H_truth == std::vector<double>(2, 0.0) && r.h_truth == std::vector<double>(2, 0.0) && r.nmi_lfk == -1.0);
  ExpectUnperturbed(fit);
  int threw = 0;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.CoverNMI(offsets, members, bad, &r); });
  EXPECT(threw == 4);
  const std::vector<std::vector<uint64_t>> bad_offsets = {{}, {1, 2}, {0, 3, 2, static_cast<uint64_t>(members.size())}, {0, 5}};
  for (const auto& bad : bad_offsets) threw += Throws([&] { learner.CoverNMI(bad, members, 0.05f, &r); });
  EXPECT(threw == 8);
  // NMI is defined on sets: a node twice inside one community is refused (twice in two communities is a cover)
  std::vector<uint32_t> twice = members;
  twice[offsets[7] + 3] = twice[offsets[7] + 2];
  threw += Throws([&] { learner.CoverNMI(offsets, twice, 0.05f, &r); });
  EXPECT(threw == 9);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/nmi.txt");
    EXPECT(learner.WriteCoverNMI(&f, offsets, members, 0.05f) && f.good());
    WriteCheckpoint(learner, d);
    WriteTruth(d, offsets, members);
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  // a member == N, a member == 2^32 - 1, an empty community and a small one; no node twice inside a community
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> members;
  SpoiltCover(PlantedCover(N), N, &offsets, &members);
  RunOnce(N, edges, offsets, members, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, offsets, members, true, nullptr);
  return Finish();
}
