// mcmc::Learner's chain average (StartAverage / GetMeanPiRow / GetMeanBeta / ReadAverage) against a float64 mean this
// program keeps itself from GetPiRow and GetBeta after every Run(1), in the synchronous loop and in the async one.
// Per entry of pi the bound is (n + 1) * 2^-22: a row is flushed at most once per step and once for the read, and a flush
// adds at most 4 * 2^-24 beside the exact recurrence (include/ammsb_average.h).  beta's mean is binary64 rounded once:
// within 2^-24 of the float64 mean.  Under ReadAverage(true) Memberships equals, exactly, a read-out of the downloaded
// mean written here.  The run itself is not perturbed, and StartAverage() throws under graph_launch.
//   average_test [DIR]   DIR is not used
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <vector>

#include "ammsb_readout.h"
#include "postfit_test.h"

namespace {

struct Rig : PreparedConfig {
  clcuda::Platform platform;
  clcuda::Device dev;
  clcuda::Context context;
  clcuda::Queue queue;
  mcmc::Learner learner;

  static mcmc::Config& Flags(mcmc::Config& c, bool async, bool graph) {
    c.device_sampling = c.async_launch = async;
    c.graph_launch = graph;
    return c;
  }
  Rig(uint64_t N, const std::vector<mcmc::Edge>& edges, bool async, bool graph)
      : PreparedConfig(N, edges, false), platform((size_t)0), dev(platform, 0), context(dev), queue(context, dev),
        learner(Flags(cfg, async, graph), queue) {}
};

template <class Call>
bool ThrowsRuntime(Call call) {
  try {
    call();
  } catch (const std::invalid_argument&) {
    return false;
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

// Memberships of a host matrix [N, K]: the statement of readout_test.cc
void ReadOut(const std::vector<mcmc::Float>& pi, uint64_t N, uint32_t K, uint32_t top, float thr, std::vector<uint32_t>* ids,
             std::vector<mcmc::Float>* weights, std::vector<uint32_t>* count, std::vector<uint64_t>* sizes) {
  ids->assign(N * top, AMMSB_READOUT_NONE);
  weights->assign(N * top, 0);
  count->assign(N, 0);
  sizes->assign(K, 0);
  std::vector<uint32_t> order(K);
  for (uint64_t a = 0; a < N; ++a) {
    const mcmc::Float* row = &pi[a * K];
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return row[x] > row[y]; });
    for (uint32_t k = 0; k < K; ++k)
      if (row[k] >= thr) {
        ++(*count)[a];
        ++(*sizes)[k];
      }
    for (uint32_t t = 0; t < top && t < K && row[order[t]] >= thr; ++t) {
      (*ids)[a * top + t] = order[t];
      (*weights)[a * top + t] = row[order[t]];
    }
  }
}

void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& edges, bool async) {
  Rig rig(N, edges, async, false);
  mcmc::Learner& learner = rig.learner;
  const uint32_t K = static_cast<uint32_t>(rig.cfg.K), warm = 5, n = 25;
  EXPECT(learner.AverageSamples() == 0);
  EXPECT(ThrowsRuntime([&] { learner.GetMeanBeta(); }));
  learner.Run(warm);
  learner.StartAverage();
  EXPECT(learner.AverageSamples() == 0);
  EXPECT(ThrowsRuntime([&] { learner.GetMeanPiRow(0); }));   // no sample yet
  std::vector<double> sum_pi(N * K, 0.0), sum_beta(2 * K, 0.0);
  std::vector<mcmc::Float> start(N * K), now(N * K);
  std::vector<char> moved(N, 0);
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
    std::copy(row.begin(), row.end(), start.begin() + a * K);
  }
  for (uint32_t t = 0; t < n; ++t) {
    learner.Run(1);
    for (uint64_t a = 0; a < N; ++a) {
      const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
      for (uint32_t k = 0; k < K; ++k) {
        sum_pi[a * K + k] += row[k];
        moved[a] |= Bits(row[k]) != Bits(start[a * K + k]);
      }
      if (t + 1 == n) std::copy(row.begin(), row.end(), now.begin() + a * K);
    }
    const std::vector<mcmc::Float> beta = learner.GetBeta();
    for (uint32_t i = 0; i < 2 * K; ++i) sum_beta[i] += beta[i];
  }
  EXPECT(learner.AverageSamples() == n);
  const double bound = (n + 1) * std::ldexp(1.0, -22);
  double worst = 0;
  uint64_t still = 0, still_bad = 0;
  std::vector<mcmc::Float> mean(N * K);
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<mcmc::Float> row = learner.GetMeanPiRow(static_cast<mcmc::Vertex>(a));
    std::copy(row.begin(), row.end(), mean.begin() + a * K);
    for (uint32_t k = 0; k < K; ++k) worst = std::max(worst, std::fabs(row[k] - sum_pi[a * K + k] / n));
    if (!moved[a]) {  // a row no mini-batch held: the mean is the row, bit for bit
      ++still;
      for (uint32_t k = 0; k < K; ++k) still_bad += Bits(row[k]) != Bits(now[a * K + k]);
    }
  }
  EXPECT(worst <= bound);
  EXPECT(still > 0 && still < N && still_bad == 0);
  const std::vector<mcmc::Float> mean_beta = learner.GetMeanBeta();
  double worst_beta = 0;
  for (uint32_t i = 0; i < 2 * K; ++i) worst_beta = std::max(worst_beta, std::fabs(mean_beta[i] - sum_beta[i] / n));
  EXPECT(mean_beta.size() == 2 * K && worst_beta <= std::ldexp(1.0, -24));
  printf("average %s: n = %u, max |mean - dense| = %.3g (bound %.3g), beta %.3g, %llu rows never in a mini-batch\n",
         async ? "async" : "sync", n, worst, bound, worst_beta, (unsigned long long)still);

  // the analyses read the mean while ReadAverage(true) is set, the last draw otherwise
  std::vector<uint32_t> ids, count, want_ids, want_count;
  std::vector<mcmc::Float> weights, want_weights;
  std::vector<uint64_t> sizes, want_sizes;
  learner.ReadAverage(true);
  learner.Memberships(4, 0.02f, &ids, &weights, &count, &sizes);
  ReadOut(mean, N, K, 4, 0.02f, &want_ids, &want_weights, &want_count, &want_sizes);
  EXPECT(ids == want_ids && SameBits(weights, want_weights) && count == want_count && sizes == want_sizes);
  learner.ReadAverage(false);
  learner.Memberships(4, 0.02f, &ids, &weights, &count, &sizes);
  ReadOut(now, N, K, 4, 0.02f, &want_ids, &want_weights, &want_count, &want_sizes);
  EXPECT(ids == want_ids && SameBits(weights, want_weights) && count == want_count && sizes == want_sizes);
  EXPECT(!SameBits(mean, now));

  // averaging and reading did not perturb the run
  {
    mcmc::Learner plain(rig.cfg, rig.queue);
    plain.Run(warm + n);
    EXPECT(learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
    EXPECT(learner.GetBeta() == plain.GetBeta() && learner.GetPiRow(17) == plain.GetPiRow(17));
  }
  // a restart counts from 0; without an average the read of the mean is refused
  learner.StartAverage();
  EXPECT(learner.AverageSamples() == 0);
  learner.Run(2);
  EXPECT(learner.AverageSamples() == 2 && learner.GetMeanPiRow(3).size() == K);
  learner.StopAverage();
  EXPECT(learner.AverageSamples() == 0);
  learner.ReadAverage(true);
  EXPECT(ThrowsRuntime([&] { learner.Memberships(4, 0.02f, &ids, &weights, &count, &sizes); }));
  learner.ReadAverage(false);
}

}  // namespace

int main(int, char**) {
  const uint64_t N = 2000;
  const std::vector<mcmc::Edge> edges = mcmc::GenerateSyntheticGraph(N, 16, 16, 7);
  EXPECT(edges.size() > 5000);
  RunOnce(N, edges, false);
  RunOnce(N, edges, true);
  {
    Rig graph(N, edges, true, true);
    EXPECT(Throws([&] { graph.learner.StartAverage(); }));
    EXPECT(graph.learner.AverageSamples() == 0);
  }
  return Finish();
}
