// mcmc::Learner's chain spread (StartAverage(true) / GetVarPiRow / GetVarBeta / ReadBound), in the synchronous loop and in
// the async one.  The program records every sample (GetPiRow and GetBeta after every Run(1)) and writes, per loop, what the
// Python side needs to replay the chain through the numpy statement of include/ammsb_spread.h and compare bits
// (tests/spread_child.py):
//   DIR/<loop>.samples   u32 N, K, n, then n times (pi [N, K] f32, beta [2K] f32)
//   DIR/<loop>.moments   mean [N, K] f32 (GetMeanPiRow), var [N, K] f32 (GetVarPiRow), var beta [2K] f64 (GetVarBeta)
//   DIR/<loop>.quality   WriteCommunityQuality(0.05) under ReadAverage(true) + ReadBound(true, -2)
//   DIR/links.txt        the training links
// Checked here: var >= 0 and within the header's bound of the float64 variance of the recorded samples, a row no mini-batch
// held has var 0, the mean is what a plain average of the same seed keeps (bit for bit), Memberships under ReadBound equals
// a read-out of the bound written here, ReadBound(true, 0) reads what ReadAverage alone does, the refusals, and that the
// run is not perturbed.
//   spread_test DIR
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "postfit_test.h"

namespace {

struct Rig : PreparedConfig {
  clcuda::Platform platform;
  clcuda::Device dev;
  clcuda::Context context;
  clcuda::Queue queue;
  mcmc::Learner learner;

  static mcmc::Config& Flags(mcmc::Config& c, bool async) {
    c.device_sampling = c.async_launch = async;
    c.graph_launch = false;
    return c;
  }
  Rig(uint64_t N, const std::vector<mcmc::Edge>& edges, bool async)
      : PreparedConfig(N, edges, false), platform((size_t)0), dev(platform, 0), context(dev), queue(context, dev),
        learner(Flags(cfg, async), queue) {}
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

template <class T>
void Put(std::ofstream& f, const std::vector<T>& v) {
  f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

// the bound of include/ammsb_spread.h: binary64's square root rounded once more is the correctly rounded binary32 one
float BoundOf(float m, float v, float z) {
  const float root = static_cast<float>(std::sqrt(static_cast<double>(v)));
  volatile float prod = z * root;  // (separately rounded: no contraction into the add)
  const float t = m + prod;
  return t > 0.0f ? std::min(t, 1.0f) : 0.0f;
}

void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& edges, bool async, const std::string& dir) {
  Rig rig(N, edges, async);
  mcmc::Learner& learner = rig.learner;
  const uint32_t K = static_cast<uint32_t>(rig.cfg.K), warm = 5, n = 20;
  const std::string stem = dir + (async ? "/async" : "/sync");
  learner.Run(warm);
  learner.StartAverage();   // no spread: the reads of the variance are refused
  learner.Run(1);
  EXPECT(ThrowsRuntime([&] { learner.GetVarPiRow(0); }) && ThrowsRuntime([&] { learner.GetVarBeta(); }));
  learner.StopAverage();
  EXPECT(Throws([&] { learner.ReadBound(true, NAN); }));

  // a second learner of the same seed keeps the plain average over the same iterations
  mcmc::Learner plain(rig.cfg, rig.queue);
  plain.Run(warm + 1);
  plain.StartAverage();
  learner.StartAverage(true);
  EXPECT(learner.AverageSamples() == 0 && ThrowsRuntime([&] { learner.GetVarPiRow(0); }));   // no sample yet

  std::ofstream samples(stem + ".samples", std::ios::binary);
  Put(samples, std::vector<uint32_t>{static_cast<uint32_t>(N), K, n});
  std::vector<double> sum(N * K, 0.0), sq(N * K, 0.0), bsum(2 * K, 0.0), bsq(2 * K, 0.0);
  std::vector<mcmc::Float> pi(N * K), first(N * K);
  std::vector<char> moved(N, 0);
  for (uint32_t t = 0; t < n; ++t) {
    learner.Run(1);
    for (uint64_t a = 0; a < N; ++a) {
      const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
      std::copy(row.begin(), row.end(), pi.begin() + a * K);
    }
    if (t == 0) first = pi;
    for (uint64_t i = 0; i < N * K; ++i) {
      sum[i] += pi[i];
      sq[i] += static_cast<double>(pi[i]) * pi[i];
      moved[i / K] |= Bits(pi[i]) != Bits(first[i]);
    }
    const std::vector<mcmc::Float> beta = learner.GetBeta();
    for (uint32_t i = 0; i < 2 * K; ++i) {
      bsum[i] += beta[i];
      bsq[i] += static_cast<double>(beta[i]) * beta[i];
    }
    Put(samples, pi);
    Put(samples, beta);
  }
  EXPECT(samples.good());
  samples.close();
  plain.Run(n);
  EXPECT(learner.AverageSamples() == n && plain.AverageSamples() == n);

  // |var - dense| <= 13 F 2^-24 + F^2 2^-43 with F <= n + 1 flushes: one per step at most, and one for the read
  const double F = n + 1, bound = 13 * F * std::ldexp(1.0, -24) + F * F * std::ldexp(1.0, -43);
  double worst = 0;
  uint64_t negative = 0, still = 0, still_bad = 0, mean_differs = 0;
  std::vector<mcmc::Float> mean(N * K), var(N * K);
  for (uint64_t a = 0; a < N; ++a) {
    const mcmc::Vertex v = static_cast<mcmc::Vertex>(a);
    const std::vector<mcmc::Float> m = learner.GetMeanPiRow(v), s = learner.GetVarPiRow(v), pm = plain.GetMeanPiRow(v);
    std::copy(m.begin(), m.end(), mean.begin() + a * K);
    std::copy(s.begin(), s.end(), var.begin() + a * K);
    for (uint32_t k = 0; k < K; ++k) {
      const double mu = sum[a * K + k] / n, dense = sq[a * K + k] / n - mu * mu;
      worst = std::max(worst, std::fabs(s[k] - dense));
      negative += !(s[k] >= 0);
      mean_differs += Bits(m[k]) != Bits(pm[k]);
      if (!moved[a]) still_bad += Bits(s[k]) != 0;
    }
    still += !moved[a];
  }
  // (the dense variance as E[x^2] - E[x]^2 in binary64 is itself good to a few 2^-53 of values <= 1)
  EXPECT(worst <= bound + 1e-14 && negative == 0 && mean_differs == 0);
  EXPECT(still > 0 && still < N && still_bad == 0);
  const std::vector<double> var_beta = learner.GetVarBeta();
  double worst_beta = 0;
  for (uint32_t i = 0; i < 2 * K; ++i) {
    const double mu = bsum[i] / n;
    worst_beta = std::max(worst_beta, std::fabs(var_beta[i] - (bsq[i] / n - mu * mu)));
  }
  EXPECT(var_beta.size() == 2 * K && worst_beta <= 1e-12);
  EXPECT(learner.GetMeanBeta() == plain.GetMeanBeta());
  printf("spread %s: n = %u, max |var - dense| = %.3g (bound %.3g), beta %.3g, %llu rows never in a mini-batch\n",
         async ? "async" : "sync", n, worst, bound, worst_beta, (unsigned long long)still);
  {
    std::ofstream f(stem + ".moments", std::ios::binary);
    Put(f, mean);
    Put(f, var);
    Put(f, var_beta);
    EXPECT(f.good());
  }

  // the analyses read the bound while ReadAverage(true) and ReadBound(true, z) are both set
  std::vector<uint64_t> size, internal, boundary, want_size(K, 0), size0, internal0, boundary0;
  uint64_t uncovered = 0, uncovered0 = 0;
  learner.ReadAverage(true);
  learner.CommunityQuality(0.05f, &size0, &internal0, &boundary0, &uncovered0);   // the mean
  learner.ReadBound(true, -2);
  learner.CommunityQuality(0.05f, &size, &internal, &boundary, &uncovered);
  for (uint64_t i = 0; i < N * K; ++i) want_size[i % K] += BoundOf(mean[i], var[i], -2.0f) >= 0.05f;
  EXPECT(size == want_size && size != size0);
  {
    std::ofstream f(stem + ".quality");
    EXPECT(learner.WriteCommunityQuality(&f, 0.05f) && f.good());
  }
  learner.ReadBound(true, 0);   // z = 0: the clamped mean, which is the mean
  learner.CommunityQuality(0.05f, &size, &internal, &boundary, &uncovered);
  EXPECT(size == size0 && internal == internal0 && boundary == boundary0 && uncovered == uncovered0);
  learner.ReadBound(true, -2);
  learner.ReadAverage(false);   // ReadBound alone reads the last draw
  learner.CommunityQuality(0.05f, &size, &internal, &boundary, &uncovered);
  learner.ReadBound(false);
  learner.CommunityQuality(0.05f, &size0, &internal0, &boundary0, &uncovered0);
  EXPECT(size == size0 && internal == internal0 && uncovered == uncovered0);
  // ReadBound(false) gave the bound matrix back; asked again, it is allocated and filled again
  learner.ReadAverage(true);
  learner.ReadBound(true, -2);
  learner.CommunityQuality(0.05f, &size, &internal, &boundary, &uncovered);
  EXPECT(size == want_size);
  learner.ReadBound(false);
  learner.ReadAverage(false);
  if (!async) WriteTrainingLinks(learner, dir);

  // keeping the spread and reading it did not perturb the run
  EXPECT(learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
  EXPECT(learner.GetBeta() == plain.GetBeta() && learner.GetPiRow(17) == plain.GetPiRow(17));
  // a restart without the spread drops it; a bound is then refused
  learner.StartAverage();
  learner.Run(2);
  EXPECT(learner.AverageSamples() == 2 && ThrowsRuntime([&] { learner.GetVarBeta(); }));
  learner.ReadAverage(true);
  learner.ReadBound(true, -2);
  EXPECT(ThrowsRuntime([&] { learner.CommunityQuality(0.05f, &size, &internal, &boundary, &uncovered); }));
  learner.ReadBound(false);
  learner.ReadAverage(false);
  learner.StopAverage();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: spread_test DIR\n");
    return 2;
  }
  const uint64_t N = 2000;
  const std::vector<mcmc::Edge> edges = mcmc::GenerateSyntheticGraph(N, 16, 16, 7);
  EXPECT(edges.size() > 5000);
  RunOnce(N, edges, false, argv[1]);
  RunOnce(N, edges, true, argv[1]);
  return Finish();
}
