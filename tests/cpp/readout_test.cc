// mcmc::Learner::Memberships / Communities against the pi the existing accessors fetch (GetPiRow), exactly: the
// expected table is a stable sort of each row by value descending (equal values by column ascending) written here.
//   readout_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                        DIR/cpp.ckpt, DIR/memberships.bin (u32 N, K, top; f32 threshold; ids; weights; count; u64
//                        sizes) and DIR/communities.txt of the first run, for a bit-level check from the other host.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <numeric>
#include <string>
#include <vector>

#include "ammsb_readout.h"
#include "postfit_test.h"

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
  Fitted fit(N, edges, device);
  mcmc::Learner& learner = fit.learner;
  const uint32_t K = static_cast<uint32_t>(fit.cfg.K);
  Check(learner, N, K, 4, 0.0f);
  Check(learner, N, K, 16, 0.02f);
  Check(learner, N, K, 1, 0.5f);
  ExpectUnperturbed(fit);
  EXPECT(Throws([&] { learner.Memberships(17, 0.0f, nullptr, nullptr, nullptr, nullptr); }));
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
    EXPECT(f.good() && c.good());
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
