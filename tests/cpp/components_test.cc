// mcmc::Learner::CommunityComponents / WriteCommunityComponents against the statement of include/ammsb_components.h over the
// pi the existing accessor fetches (GetPiRow) and the training links: node a is a member of community k iff pi[a, k] >=
// threshold in binary32; the memberships are numbered node by node; a sequential union-find over (key, shared community)
// gives the components, whose roots are their smallest nodes.  Integers on both sides: every output is equal, and the
// float64 values, one formula over equal integers, are bit-equal.
//   components_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes
//                           DIR/cpp.ckpt, DIR/components.txt (threshold 0.05) and DIR/links.txt (the link-communities file,
//                           which lists the training links) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ammsb_components.h"
#include "postfit_test.h"
typedef mcmc::Learner::ComponentsResult Result;

static uint64_t Find(std::vector<uint64_t>& parent, uint64_t x) {
  while (parent[x] != x) {
    parent[x] = parent[parent[x]];
    x = parent[x];
  }
  return x;
}

// the statement over a list of keys -> a result whose Derive() has run
static Result Statement(const std::vector<mcmc::Float>& pi, uint64_t N, uint64_t K, float thr, const std::vector<mcmc::Edge>& keys) {
  Result w;
  w.offsets.assign(N + 1, 0);
  std::vector<int64_t> slot_of(N * K, -1);
  std::vector<uint32_t> slot_node;
  for (uint64_t a = 0; a < N; ++a) {
    for (uint64_t k = 0; k < K; ++k)
      if (pi[a * K + k] >= thr) {
        slot_of[a * K + k] = static_cast<int64_t>(slot_node.size());
        slot_node.push_back(static_cast<uint32_t>(a));
        w.community.push_back(static_cast<uint16_t>(k));
      }
    w.offsets[a + 1] = slot_node.size();
  }
  const uint64_t M = slot_node.size();
  std::vector<uint64_t> parent(M);
  for (uint64_t s = 0; s < M; ++s) parent[s] = s;
  for (mcmc::Edge e : keys) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    if (a >= N || b >= N) {
      ++w.skipped;
      continue;
    }
    ++w.links;
    for (uint64_t k = 0; k < K; ++k)
      if (slot_of[a * K + k] >= 0 && slot_of[b * K + k] >= 0) {
        ++w.shared;
        const uint64_t x = Find(parent, slot_of[a * K + k]), y = Find(parent, slot_of[b * K + k]);
        if (x != y) parent[std::max(x, y)] = std::min(x, y);
      }
  }
  std::vector<uint32_t> count(M, 0);
  for (uint64_t s = 0; s < M; ++s) ++count[Find(parent, s)];
  w.root.resize(M);
  w.size.resize(M);
  w.members.assign(K, 0);
  w.components.assign(K, 0);
  w.singletons.assign(K, 0);
  w.largest.assign(K, 0);
  w.largest_root.assign(K, -1);
  for (uint64_t s = 0; s < M; ++s) {
    const uint64_t r = Find(parent, s);
    const uint16_t k = w.community[s];
    w.root[s] = slot_node[r];
    w.size[s] = count[r];
    ++w.members[k];
    if (r != s) continue;
    ++w.components[k];
    w.singletons[k] += count[r] == 1;
    if (count[r] > w.largest[k]) {  // (slots ascend with the nodes: among equal sizes the first, the smallest root, stays)
      w.largest[k] = count[r];
      w.largest_root[k] = static_cast<int32_t>(slot_node[r]);
    }
  }
  w.stray.assign(N, 0);
  for (uint64_t s = 0; s < M; ++s) w.stray[slot_node[s]] += static_cast<int64_t>(w.root[s]) != w.largest_root[w.community[s]];
  w.Derive();
  return w;
}

static void Compare(const Result& got, const Result& want) {
  EXPECT(got.members == want.members && got.components == want.components && got.singletons == want.singletons);
  EXPECT(got.largest == want.largest && got.largest_root == want.largest_root);
  EXPECT(got.offsets == want.offsets && got.community == want.community && got.root == want.root && got.size == want.size);
  EXPECT(got.stray == want.stray);
  EXPECT(got.links == want.links && got.skipped == want.skipped && got.shared == want.shared);
  EXPECT(SameBits(got.giant, want.giant) && SameBits(got.fragmentation, want.fragmentation));
  EXPECT(memcmp(&got.connected, &want.connected, sizeof(double)) == 0);
}

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  const uint64_t N = cfg.N, K = cfg.K;
  const std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  Result got;
  learner.CommunityComponents(thr, &got);
  Compare(got, Statement(pi, N, K, thr, links));
  EXPECT(got.skipped == 0 && got.links == links.size());
  const uint64_t slots = got.root.size();
  // a list of its own: a loop, a repeat in the other order of the ends, and keys with an end >= N
  std::vector<mcmc::Edge> own;
  for (size_t i = 0; i < links.size(); i += 2) own.push_back(links[i]);
  own.push_back((7ull << 32) | 7ull);
  own.push_back(((own[3] & 0xFFFFFFFFull) << 32) | (own[3] >> 32));
  own.push_back(own[5]);
  own.push_back((static_cast<uint64_t>(N) << 32) | 1ull);
  own.push_back((2ull << 32) | 0xFFFFFFFFull);
  learner.CommunityComponents(thr, &got, &own);
  const Result want = Statement(pi, N, K, thr, own);
  Compare(got, want);
  EXPECT(got.skipped == 2 && got.links == own.size() - 2);
  uint64_t pieces = 0;
  for (uint64_t c : want.components) pieces += c;
  printf("CommunityComponents thr=%g ok: %llu slots, %llu components over the half list\n", static_cast<double>(thr),
         static_cast<unsigned long long>(slots), static_cast<unsigned long long>(pieces));
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
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.CommunityComponents(bad, &r); });
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/components.txt");
    EXPECT(learner.WriteCommunityComponents(&f, 0.05f) && f.good());
    WriteTrainingLinks(learner, d);
    WriteCheckpoint(learner, d);
  }
}

int main(int argc, char** argv) {
  // the derived values on hand-made integers: two components of two and one alone; a path of three; an empty community
  Result hand;
  hand.members = {5, 3, 0};
  hand.components = {3, 1, 0};
  hand.largest = {2, 3, 0};
  hand.Derive();
  EXPECT(hand.giant[0] == 2.0 / 5.0 && hand.giant[1] == 1.0 && hand.giant[2] == -1.0);
  EXPECT(hand.fragmentation[0] == 1.0 - 2.0 / 5.0 && hand.fragmentation[1] == 0.0 && hand.fragmentation[2] == -1.0);
  EXPECT(hand.connected == 0.5);
  hand.members = {0};
  hand.components = {0};
  hand.largest = {0};
  hand.Derive();
  EXPECT(hand.connected == -1.0 && hand.giant[0] == -1.0);

  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
