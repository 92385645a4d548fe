// mcmc::Learner::Reduce against a restatement of include/ammsb_reduce.h written here over GetPiRow / GetPhiSum / GetTheta,
// bit for bit, in the synchronous loop, the async one and the graph one: the identity, and a plan that merges and drops.
// The reduced learner steps; the old one goes on as if nothing had happened.  WritePlan / ReadPlan: the file DIR/cpp.plan
// is compared with Python's text form of the same plan by the caller.
//   reduce_test [DIR]
#include <cmath>
#include <cstdio>
#include <sstream>
#include <vector>

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

std::vector<mcmc::Float> AllPi(mcmc::Learner& l, uint64_t N) {
  std::vector<mcmc::Float> pi;
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<mcmc::Float> row = l.GetPiRow(static_cast<mcmc::Vertex>(a));
    pi.insert(pi.end(), row.begin(), row.end());
  }
  return pi;
}

// The plan of this test over 64 communities, numbered by smallest source: {3, 17, 40} and {8, 9} merged, 5 and 63 dropped.
// tests/reduce_child.py builds the same one: Plan.identity(64).merge([(3, 17), (17, 40), (8, 9)]).drop([5, 63]).
std::vector<int32_t> TestPlan(uint32_t K) {
  std::vector<int32_t> rep(K);
  for (uint32_t k = 0; k < K; ++k) rep[k] = static_cast<int32_t>(k);
  rep[17] = rep[40] = 3;
  rep[9] = 8;
  rep[5] = rep[63] = -1;
  std::vector<int32_t> number(K, -1), map(K, -1);
  int32_t next = 0;
  for (uint32_t k = 0; k < K; ++k) {
    if (rep[k] < 0) continue;
    if (number[rep[k]] < 0) number[rep[k]] = next++;   // ascending k: a group is met first at its smallest source
    map[k] = number[rep[k]];
  }
  return map;
}

// the header's statement of one row: -> emptied?
bool ReduceRow(const mcmc::Float* row, mcmc::Float phi, const std::vector<uint32_t>& off, const std::vector<uint32_t>& src,
               bool drops, mcmc::Float* out, mcmc::Float* out_phi) {
  const uint32_t new_K = static_cast<uint32_t>(off.size() - 1);
  std::vector<mcmc::Float> t(new_K);
  for (uint32_t j = 0; j < new_K; ++j) {
    mcmc::Float s = row[src[off[j]]];
    for (uint32_t p = off[j] + 1; p < off[j + 1]; ++p) s = s + row[src[p]];
    t[j] = s;
  }
  *out_phi = phi;
  if (!drops) {
    std::copy(t.begin(), t.end(), out);
    return false;
  }
  double x[64];
  for (double& v : x) v = 0.0;
  for (uint32_t j = 0; j < new_K; ++j) x[j & 63u] = x[j & 63u] + static_cast<double>(t[j]);
  for (uint32_t d = 32; d > 0; d >>= 1)
    for (uint32_t v = 0; v < d; ++v) x[v] = x[v] + x[v + d];
  const mcmc::Float sf = static_cast<mcmc::Float>(x[0]);
  if (!(sf > 0)) {
    for (uint32_t j = 0; j < new_K; ++j) out[j] = 1.0f / static_cast<mcmc::Float>(new_K);
    return true;
  }
  for (uint32_t j = 0; j < new_K; ++j) out[j] = t[j] / sf;
  *out_phi = phi * sf;
  return false;
}

void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& edges, bool async, bool graph, const char* dir) {
  Rig rig(N, edges, async, graph);
  mcmc::Learner& learner = rig.learner;
  const uint32_t K = static_cast<uint32_t>(rig.cfg.K);
  learner.Run(30);
  const std::vector<mcmc::Float> pi = AllPi(learner, N), phi = learner.GetPhiSum(), theta = learner.GetTheta(), beta = learner.GetBeta();

  // the identity: the same model bit for bit, at the same point of the schedule
  {
    std::vector<int32_t> ident(K);
    for (uint32_t k = 0; k < K; ++k) ident[k] = static_cast<int32_t>(k);
    std::unique_ptr<mcmc::Learner> same = learner.Reduce(ident);
    EXPECT(SameBits(AllPi(*same, N), pi) && SameBits(same->GetPhiSum(), phi) && SameBits(same->GetTheta(), theta));
    EXPECT(SameBits(same->GetBeta(), beta));
    EXPECT(same->ReducedFromK() == K && same->EmptiedRows() == 0 && learner.ReducedFromK() == 0);
    EXPECT(same->MiniBatchEdges() == learner.MiniBatchEdges());
  }

  const std::vector<int32_t> map = TestPlan(K);
  std::vector<uint32_t> off, src;
  mcmc::PlanSources(map, &off, &src);
  const uint32_t new_K = static_cast<uint32_t>(off.size() - 1);
  EXPECT(new_K == K - 5 && src.size() == K - 2);
  std::unique_ptr<mcmc::Learner> red = learner.Reduce(map);
  std::vector<mcmc::Float> want_pi(N * new_K), want_phi(N), want_theta(2 * new_K);
  uint64_t emptied = 0;
  for (uint64_t a = 0; a < N; ++a) emptied += ReduceRow(&pi[a * K], phi[a], off, src, true, &want_pi[a * new_K], &want_phi[a]);
  for (uint32_t j = 0; j < new_K; ++j)
    for (uint32_t i = 0; i < 2; ++i) {
      mcmc::Float s = theta[2 * src[off[j]] + i];
      for (uint32_t p = off[j] + 1; p < off[j + 1]; ++p) s = s + theta[2 * src[p] + i];
      want_theta[2 * j + i] = s;
    }
  EXPECT(SameBits(AllPi(*red, N), want_pi));
  EXPECT(SameBits(red->GetPhiSum(), want_phi));
  EXPECT(SameBits(red->GetTheta(), want_theta));
  EXPECT(red->ReducedFromK() == K && red->EmptiedRows() == emptied);
  const std::vector<mcmc::Float> red_beta = red->GetBeta();
  EXPECT(red_beta.size() == 2 * new_K);
  // the learner itself is untouched
  EXPECT(SameBits(AllPi(learner, N), pi) && SameBits(learner.GetTheta(), theta) && SameBits(learner.GetBeta(), beta));

  // the reduced learner steps, from the old one's count of mini-batch edges on
  const uint64_t edges_before = red->MiniBatchEdges();
  const mcmc::Float ppx0 = red->HeldoutPerplexity();
  red->Run(5);
  const mcmc::Float ppx1 = red->HeldoutPerplexity();
  EXPECT(edges_before == learner.MiniBatchEdges() && red->MiniBatchEdges() > edges_before);
  EXPECT(std::isfinite(ppx0) && std::isfinite(ppx1) && red->GetPiRow(17).size() == new_K);
  EXPECT(!SameBits(red->GetTheta(), want_theta));
  printf("reduce %s: K = %u -> %u, %llu emptied rows, held-out perplexity %.4f reduced, %.4f after 5 steps\n",
         graph ? "graph" : async ? "async" : "sync", K, new_K, (unsigned long long)emptied, ppx0, ppx1);
  red.reset();

  // Run(30), Reduce, Run(30) leaves what Run(60) leaves
  {
    mcmc::Learner plain(rig.cfg, rig.queue);
    plain.Run(60);
    learner.Run(30);
    EXPECT(learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
    EXPECT(learner.GetBeta() == plain.GetBeta() && learner.GetPiRow(17) == plain.GetPiRow(17));
  }

  // refusals
  std::vector<int32_t> bad = map;
  bad.pop_back();
  EXPECT(Throws([&] { learner.Reduce(bad); }));                       // another K
  bad = map;
  bad[0] = static_cast<int32_t>(K);
  EXPECT(Throws([&] { learner.Reduce(bad); }));                       // outside -1 .. K - 1
  bad = map;
  for (auto& m : bad) m = m == 7 ? 8 : m;
  EXPECT(Throws([&] { learner.Reduce(bad); }));                       // new community 7 has no source
  bad.assign(K, -1);
  EXPECT(Throws([&] { learner.Reduce(bad); }));                       // nothing left

  if (dir) {
    const std::string path = std::string(dir) + "/cpp.plan";
    {
      std::ofstream pf(path);
      EXPECT(mcmc::WritePlan(&pf, map) && pf.good());
    }
    std::ifstream in(path);
    EXPECT(mcmc::ReadPlan(&in) == map);
    std::istringstream odd("# 5 3 1\n0 2 1 2\n1 1 4\n2 1 0\nx 3\n");   // not numbered by smallest source: kept as written
    EXPECT((mcmc::ReadPlan(&odd) == std::vector<int32_t>{2, 0, 0, -1, 1}));
    for (const char* text : {"", "# 3 2\n", "# 3 2 0\n0 2 0 1\n", "# 3 2 0\n0 2 0 1\n1 1 1\n", "# 3 2 0\n0 2 0 1\n1 1 3\n",
                             "# 3 2 0\n1 2 0 1\n0 1 2\n", "# 3 2 1\n0 1 0\n1 1 1\nx 2\nx 2\n", "# 3 1 0\n0 3 0 1\n",
                             "# 3 2 0\n0 2 0 one\n1 1 2\n"}) {
      std::istringstream s(text);
      EXPECT(Throws([&] { mcmc::ReadPlan(&s); }));
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t N = 2000;
  const std::vector<mcmc::Edge> edges = mcmc::GenerateSyntheticGraph(N, 16, 16, 7);
  EXPECT(edges.size() > 5000);
  RunOnce(N, edges, false, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, false, nullptr);
  RunOnce(N, edges, true, true, nullptr);
  return Finish();
}
