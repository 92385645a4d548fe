// mcmc::Learner::CommunityCores / WriteCommunityCores against the statement of include/ammsb_cores.h over the pi the existing
// accessor fetches (GetPiRow) and the training links: node a is a member of community k iff pi[a, k] >= threshold in
// binary32; the memberships are numbered node by node; the simple adjacency induces a graph on them, whose core numbers the
// bucket peeling of Batagelj and Zaversnik gives.  Integers on both sides: every output is equal, and the float64 values, one
// formula over equal integers, are bit-equal.
//   cores_test [DIR]   synchronous loop, then device sampling + async + graph launch; with DIR it also writes DIR/cpp.ckpt,
//                      DIR/cores.txt (threshold 0.05) and DIR/links.txt (the link-communities file, which lists the training
//                      links) of the first run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include "ammsb_cores.h"
#include "postfit_test.h"
typedef mcmc::Learner::CoresResult Result;

// the statement over a list of keys -> a result whose Derive() has run
static Result Statement(const std::vector<mcmc::Float>& pi, uint64_t N, uint64_t K, float thr, const std::vector<mcmc::Edge>& keys) {
  Result w;
  // the simple adjacency
  std::vector<std::set<uint32_t>> rows(N);
  uint64_t valid = 0, entries = 0;
  for (mcmc::Edge e : keys) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    if (a >= N || b >= N) {
      ++w.skipped;
      continue;
    }
    ++valid;
    if (a == b) continue;
    rows[a].insert(static_cast<uint32_t>(b));
    rows[b].insert(static_cast<uint32_t>(a));
  }
  for (uint64_t a = 0; a < N; ++a) entries += rows[a].size();
  w.dropped = valid - entries / 2;
  // the slots
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
  // the induced slot graph
  std::vector<std::vector<uint32_t>> nbr(M);
  for (uint64_t s = 0; s < M; ++s)
    for (uint32_t b : rows[slot_node[s]]) {
      const int64_t t = slot_of[static_cast<uint64_t>(b) * K + w.community[s]];
      if (t >= 0) nbr[s].push_back(static_cast<uint32_t>(t));
    }
  w.indeg.resize(M);
  uint32_t md = 0;
  for (uint64_t s = 0; s < M; ++s) {
    w.indeg[s] = static_cast<uint32_t>(nbr[s].size());
    w.L += nbr[s].size();
    md = std::max(md, w.indeg[s]);
  }
  // bucket peeling: the vertices in bins by degree; the one of the smallest degree leaves and every neighbour of a larger
  // degree moves one bin down
  std::vector<uint32_t> deg(w.indeg);
  std::vector<uint64_t> start(md + 2, 0), pos(M), vert(M);
  for (uint64_t s = 0; s < M; ++s) ++start[deg[s] + 1];
  for (uint32_t d = 1; d < md + 2; ++d) start[d] += start[d - 1];
  std::vector<uint64_t> place(start.begin(), start.end() - 1);
  for (uint64_t s = 0; s < M; ++s) {
    pos[s] = place[deg[s]]++;
    vert[pos[s]] = s;
  }
  for (uint64_t i = 0; i < M; ++i) {
    const uint64_t v = vert[i];
    for (uint32_t u : nbr[v])
      if (deg[u] > deg[v]) {
        const uint32_t du = deg[u];
        const uint64_t pu = pos[u], pw = start[du], x = vert[pw];
        if (u != x) {
          pos[u] = pw;
          pos[x] = pu;
          vert[pu] = x;
          vert[pw] = u;
        }
        ++start[du];
        --deg[u];
      }
  }
  w.core = deg;
  w.members.assign(K, 0);
  w.inlinks2.assign(K, 0);
  w.nucleus.assign(K, 0);
  w.isolated.assign(K, 0);
  w.degeneracy.assign(K, 0);
  for (uint64_t s = 0; s < M; ++s) {
    const uint16_t k = w.community[s];
    ++w.members[k];
    w.inlinks2[k] += w.indeg[s];
    w.isolated[k] += w.core[s] == 0;
    w.degeneracy[k] = std::max(w.degeneracy[k], w.core[s]);
  }
  w.best_core.assign(N, 0);
  w.best_comm.assign(N, -1);
  w.in_nucleus.assign(N, 0);
  for (uint64_t s = 0; s < M; ++s) {
    const uint16_t k = w.community[s];
    const uint32_t a = slot_node[s];
    if (w.core[s] == w.degeneracy[k]) {
      ++w.nucleus[k];
      w.in_nucleus[a] += w.degeneracy[k] > 0;
    }
    if (w.best_comm[a] < 0 || w.core[s] > w.best_core[a]) {  // (slots ascend with k: among equals the first stays)
      w.best_core[a] = w.core[s];
      w.best_comm[a] = k;
    }
  }
  w.Derive();
  return w;
}

static void Compare(const Result& got, const Result& want) {
  EXPECT(got.members == want.members && got.inlinks2 == want.inlinks2 && got.degeneracy == want.degeneracy);
  EXPECT(got.nucleus == want.nucleus && got.isolated == want.isolated);
  EXPECT(got.offsets == want.offsets && got.community == want.community && got.indeg == want.indeg && got.core == want.core);
  EXPECT(got.best_core == want.best_core && got.best_comm == want.best_comm && got.in_nucleus == want.in_nucleus);
  EXPECT(got.L == want.L && got.skipped == want.skipped && got.dropped == want.dropped);
  EXPECT(SameBits(got.coreness, want.coreness) && SameBits(got.nucleus_share, want.nucleus_share) &&
         SameBits(got.mean_core, want.mean_core));
  std::set<uint32_t> distinct(want.core.begin(), want.core.end());
  EXPECT(got.rounds <= want.core.size() && got.scans <= 2 * distinct.size() + 1);
}

static void Check(mcmc::Learner& learner, const mcmc::Config& cfg, const std::vector<mcmc::Float>& pi, float thr) {
  const uint64_t N = cfg.N, K = cfg.K;
  const std::vector<mcmc::Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  Result got;
  learner.CommunityCores(thr, &got);
  Compare(got, Statement(pi, N, K, thr, links));
  EXPECT(got.skipped == 0 && got.dropped == 0);
  // a list of its own: a loop, a repeat in the other order of the ends, and keys with an end >= N
  std::vector<mcmc::Edge> own;
  for (size_t i = 0; i < links.size(); i += 2) own.push_back(links[i]);
  own.push_back((7ull << 32) | 7ull);
  own.push_back(((own[3] & 0xFFFFFFFFull) << 32) | (own[3] >> 32));
  own.push_back(own[5]);
  own.push_back((static_cast<uint64_t>(N) << 32) | 1ull);
  own.push_back((2ull << 32) | 0xFFFFFFFFull);
  learner.CommunityCores(thr, &got, &own);
  const Result want = Statement(pi, N, K, thr, own);
  Compare(got, want);
  EXPECT(got.skipped == 2 && got.dropped == 3);
  uint32_t top = 0;
  for (uint32_t d : want.degeneracy) top = std::max(top, d);
  printf("CommunityCores thr=%g ok: %llu slots, %llu entries, degeneracy up to %u, %llu scans, %llu rounds\n",
         static_cast<double>(thr), static_cast<unsigned long long>(got.core.size()), static_cast<unsigned long long>(got.L), top,
         static_cast<unsigned long long>(got.scans), static_cast<unsigned long long>(got.rounds));
  // the neighbour lists against max_bytes: refused, and the message names the threshold
  if (got.L > 1) {
    bool named = false;
    try {
      learner.CommunityCores(thr, &got, &own, 4 * got.L - 4);
    } catch (const std::invalid_argument& e) {
      named = std::string(e.what()).find("max_bytes is " + std::to_string(4 * want.L - 4)) != std::string::npos &&
              std::string(e.what()).find("threshold") != std::string::npos;
    }
    EXPECT(named);
  }
}

static void RunOnce(uint64_t N, const std::vector<mcmc::Edge>& graph, bool device, const char* dir) {
  Fitted fit(N, graph, device);
  mcmc::Learner& learner = fit.learner;
  const mcmc::Config& cfg = fit.cfg;
  const std::vector<mcmc::Float> pi = fit.Pi();
  Check(learner, cfg, pi, 0.05f);
  Check(learner, cfg, pi, 1.0f / 64);
  ExpectUnperturbed(fit);
  int threw = 0;
  Result r;
  for (float bad : {-1e-9f, -1.0f, NAN, INFINITY}) threw += Throws([&] { learner.CommunityCores(bad, &r); });
  EXPECT(threw == 4);
  if (dir) {
    const std::string d(dir);
    // (the learner has moved on: the file and the checkpoint are of the same, current state)
    std::ofstream f(d + "/cores.txt");
    EXPECT(learner.WriteCommunityCores(&f, 0.05f) && f.good());
    WriteTrainingLinks(learner, d);
    WriteCheckpoint(learner, d);
  }
}

int main(int argc, char** argv) {
  // the derived values on hand-made integers: a triangle with a pendant member and one alone; a path of three; an empty
  // community
  Result hand;
  hand.members = {5, 3, 0};
  hand.nucleus = {3, 3, 0};
  hand.degeneracy = {2, 1, 0};
  hand.community = {0, 0, 0, 0, 1, 1, 1, 0};
  hand.core = {2, 2, 2, 1, 1, 1, 1, 0};
  hand.Derive();
  EXPECT(hand.coreness[0] == 1.0 && hand.coreness[3] == 0.5 && hand.coreness[7] == 0.0 && hand.coreness[4] == 1.0);
  EXPECT(hand.nucleus_share[0] == 3.0 / 5.0 && hand.nucleus_share[1] == 1.0 && hand.nucleus_share[2] == -1.0);
  EXPECT(hand.mean_core[0] == 7.0 / 5.0 && hand.mean_core[1] == 1.0 && hand.mean_core[2] == -1.0);
  hand.degeneracy = {0, 0, 0};
  hand.core.assign(8, 0);
  hand.Derive();
  EXPECT(hand.coreness[0] == -1.0 && hand.mean_core[0] == 0.0);

  const uint64_t N = 20000;
  const std::vector<mcmc::Edge> edges = TestGraph(N);
  RunOnce(N, edges, false, argc > 1 ? argv[1] : nullptr);
  RunOnce(N, edges, true, nullptr);
  return Finish();
}
