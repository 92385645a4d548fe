// mcmc::Learner::Memberships / Communities against the pi the existing accessors fetch (GetPiRow), exactly: the
// expected table is a stable sort of each row by value descending (equal values by column ascending) written here.
//   readout_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                        DIR/cpp.ckpt, DIR/memberships.bin (u32 N, K, top; f32 threshold; ids; weights; count; u64
//                        sizes) and DIR/communities.txt of the first run, for a bit-level check from the other host.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "ammsb_readout.h"
#include "mcmc/data.h"
#include "mcmc/learner.h"

namespace clcuda = mcmc::clcuda;

static int fails = 0;
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);   \
      ++fails;                                                \
    }                                                         \
  } while (0)

static bool Prepare(mcmc::Config* cfg, uint64_t N, std::vector<mcmc::Edge> e) {
  cfg->N = N;
  cfg->K = 64;
  cfg->mini_batch_size = 256;
  cfg->num_node_sample = 16;
  cfg->heldout_ratio = 0.05;
  cfg->alpha = static_cast<mcmc::Float>(1) / cfg->K;
  cfg->phi_wg_size = cfg->beta_wg_size = cfg->ppx_wg_size = 64;
  cfg->beta_seed = {44, 45};
  cfg->neighbor_seed = {56, 57};
  srand(12345);
  bool ok = false;
  for (int attempt = 0; attempt < 64 && !ok; ++attempt) {
    cfg->training_edges.clear();
    cfg->heldout_edges.clear();
    ok = mcmc::GenerateSetsFromEdges(cfg->N, e, cfg->heldout_ratio, &cfg->training_edges, &cfg->heldout_edges,
                                     &cfg->training, &cfg->heldout);
    if (!ok) e.resize(e.size() - 40);
  }
  if (!ok) return false;
  cfg->trainingGraph.reset(new mcmc::Graph(cfg->N, cfg->training_edges));
  cfg->heldoutGraph.reset(new mcmc::Graph(cfg->N, cfg->heldout_edges));
  cfg->E = e.size();
  return true;
}

static uint32_t Bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static void Check(mcmc::Learner& learner, uint64_t N, uint32_t K, uint32_t top, float thr) {
  std::vector<uint32_t> ids, count;
  std::vector<mcmc::Float> weights;
  std::vector<uint64_t> sizes;
  learner.Memberships(top, thr, &ids, &weights, &count, &sizes);
  EXPECT(ids.size() == N * top && weights.size() == N * top && count.size() == N && sizes.size() == K);
  std::vector<uint64_t> want_sizes(K, 0);
  std::vector<uint32_t> order(K);
  uint64_t bad = 0;
  for (uint64_t a = 0; a < N; ++a) {
    const std::vector<mcmc::Float> row = learner.GetPiRow(static_cast<mcmc::Vertex>(a));
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return row[x] > row[y]; });
    uint32_t c = 0;
    for (uint32_t k = 0; k < K; ++k)
      if (row[k] >= thr) {
        ++c;
        ++want_sizes[k];
      }
    bad += count[a] != c;
    for (uint32_t t = 0; t < top; ++t) {
      const bool have = t < K && row[order[t]] >= thr;
      const uint32_t id = have ? order[t] : AMMSB_READOUT_NONE;
      const uint32_t w = have ? Bits(row[order[t]]) : 0u;
      bad += ids[a * top + t] != id || Bits(weights[a * top + t]) != w;
    }
  }
  EXPECT(bad == 0);
  EXPECT(sizes == want_sizes);
  // the communities view of the same table
  std::vector<uint64_t> offsets, sizes2;
  std::vector<uint32_t> members;
  learner.Communities(top, thr, &offsets, &members, &sizes2);
  EXPECT(sizes2 == want_sizes && offsets.size() == K + 1u && offsets[K] == members.size());
  uint64_t listed = 0;
  for (uint32_t id : ids) listed += id != AMMSB_READOUT_NONE;
  EXPECT(listed == members.size());
  for (uint32_t k = 0; k < K; ++k) {
    EXPECT(offsets[k + 1] - offsets[k] <= sizes2[k]);
    for (uint64_t i = offsets[k]; i < offsets[k + 1]; ++i) {
      if (i > offsets[k]) EXPECT(members[i - 1] < members[i]);
      const uint32_t* slots = &ids[static_cast<uint64_t>(members[i]) * top];
      EXPECT(std::find(slots, slots + top, k) != slots + top);
    }
  }
  printf("readout top=%u thr=%g: %llu slots listed, mismatches %llu\n", top, thr, (unsigned long long)listed,
         (unsigned long long)bad);
}

template <class T>
static void Put(std::ofstream& f, const std::vector<T>& v) {
  f.write(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(T));
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& edges, bool device, const char* dir) {
  mcmc::Config cfg;
  cfg.device_sampling = cfg.async_launch = cfg.graph_launch = device;
  EXPECT(Prepare(&cfg, N, edges));
  clcuda::Platform platform((size_t)0);
  clcuda::Device dev(platform, 0);
  clcuda::Context context(dev);
  clcuda::Queue queue(context, dev);
  mcmc::Learner learner(cfg, queue);
  learner.Run(30);
  const uint32_t K = static_cast<uint32_t>(cfg.K);
  Check(learner, N, K, 4, 0.0f);
  Check(learner, N, K, 16, 0.02f);
  Check(learner, N, K, 1, 0.5f);
  // reading out does not perturb the run: the state after 30 more steps equals that of an undisturbed learner
  mcmc::Learner plain(cfg, queue);
  plain.Run(30);
  plain.Run(30);
  learner.Run(30);
  EXPECT(learner.HeldoutPerplexity() == plain.HeldoutPerplexity());
  EXPECT(learner.GetBeta() == plain.GetBeta() && learner.GetPiRow(17) == plain.GetPiRow(17));
  bool threw = false;
  try {
    learner.Memberships(17, 0.0f, nullptr, nullptr, nullptr, nullptr);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  if (dir) {
    const std::string d(dir);
    const uint32_t top = 4;
    const float thr = 0.05f;
    std::vector<uint32_t> ids, count;
    std::vector<mcmc::Float> weights;
    std::vector<uint64_t> sizes;
    learner.Memberships(top, thr, &ids, &weights, &count, &sizes);
    std::ofstream f(d + "/memberships.bin", std::ios::binary);
    const uint32_t head[3] = {static_cast<uint32_t>(N), K, top};
    f.write(reinterpret_cast<const char*>(head), sizeof(head));
    f.write(reinterpret_cast<const char*>(&thr), 4);
    Put(f, ids);
    Put(f, weights);
    Put(f, count);
    Put(f, sizes);
    std::ofstream c(d + "/communities.txt");
    EXPECT(learner.WriteCommunities(&c, top, thr));
    std::ofstream ck(d + "/cpp.ckpt", std::ios::binary);
    EXPECT(learner.Serialize(&ck));
    EXPECT(f.good() && c.good() && ck.good());
  }
}

int main(int argc, char** argv) {
  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = mcmc::GenerateSyntheticGraph(N, 16, 16, 7);
  EXPECT(edges.size() > 100000);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  printf(fails ? "FAILED (%d)\n" : "OK\n", fails);
  return fails ? 1 : 0;
}
