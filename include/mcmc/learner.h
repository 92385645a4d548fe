// mcmc::Learner: drop-in for the reference's mcmc/learner.h:18-88 (same constructor, same methods).
#ifndef MCMC_AMD_LEARNER_H_
#define MCMC_AMD_LEARNER_H_

#include <signal.h>

#include <future>
#include <map>
#include <istream>
#include <memory>
#include <ostream>
#include <random>

#include "mcmc/config.h"
#include "mcmc/data.h"
#include "mcmc/operators.h"

namespace mcmc {

class Learner {
 public:
  Learner(const Config& cfg, clcuda::Queue queue);
  ~Learner();

  void Run(uint32_t max_iters, sig_atomic_t* signaled = nullptr);  // learner.cc:214-250
  Float HeldoutPerplexity();                                       // learner.cc:196-203
  Float TrainingPerplexity();                                      // learner.cc:204-212 (Config::calc_train_ppx)
  void PrintStats(std::ostream& out);                              // learner.cc:252-299
  void PrintStats();
  bool Serialize(std::ostream* out);  // learner.cc:301-330
  bool Parse(std::istream* in);       // learner.cc:332-363

  // read-back helpers for tests / drivers (not in the reference API)
  std::vector<Float> GetBeta();
  std::vector<Float> GetTheta();
  std::vector<Float> GetPiRow(Vertex v);
  uint64_t MiniBatchEdges() const { return edges_done_; }

  // Averaging over the chain (include/ammsb_average.h; not in the reference API).  From StartAverage() on the learner keeps
  // the mean of (pi, beta) over the iterations: sample t is the state after the t-th Step since.  The mean of pi is lazy -- a
  // row is brought up to date just before an iteration overwrites it (first thing in Step) and once more when the mean is
  // read -- and costs a second pi in device memory; beta's mean is kept in binary64 (last thing in Step).  Both the
  // synchronous and the async loop keep it.  StartAverage() again sets the count back to 0; Parse() ends the average (the
  // checkpoint does not carry it).  Throws std::invalid_argument under Config::graph_launch and when the run is sharded.
  // spread = true keeps the population variance of every entry of pi (lazily, in the same flush) and of beta (Welford, in
  // binary64) beside the mean (include/ammsb_spread.h): a third pi in device memory.  mean and beta's mean keep their bits.
  void StartAverage(bool spread = false);
  void StopAverage();
  uint32_t AverageSamples() const { return averaging_ ? avg_n_ : 0; }
  // the mean of beta rounded to binary32 once, and a row of the mean of pi; both flush first and throw std::runtime_error
  // while no sample exists
  std::vector<Float> GetMeanBeta();
  std::vector<Float> GetMeanPiRow(Vertex v);
  // While set, every post-fit method below reads the flushed mean of (pi, beta) instead of the last draw (and throws
  // std::runtime_error while no sample exists).  Off by default.
  void ReadAverage(bool on) { read_average_ = on; }
  // With the spread on: beta's population variance m2 / n in binary64 and a row of pi's variance; both flush first and throw
  // std::runtime_error without a spread or a sample.
  std::vector<double> GetVarBeta();
  std::vector<Float> GetVarPiRow(Vertex v);
  // While set together with ReadAverage(true), every post-fit method reads the credible bound clamp(mean + z sd, 0, 1) of pi
  // (z < 0: the lower bound; a fourth pi in device memory, refilled only when samples have arrived since) and the mean of
  // beta.  ReadBound(false) frees that matrix.  The rows of a bound do not sum to 1: link scores on it are conservative
  // scores, not probabilities.  Throws
  // std::invalid_argument on a z that is not finite; the post-fit methods throw std::runtime_error without a spread.
  void ReadBound(bool on, Float z = -2);

  // Fewer communities (include/ammsb_reduce.h; not in the reference API).  map[K]: map[k] = j sends community k to the new
  // community j in [0, K'), -1 drops it; every new community needs a source.  -> a new learner over the same data (it owns a
  // copy of the Config with K = K', alpha as this Config holds it) and the same queue, whose pi, phi_sum and theta are this
  // learner's under the plan and whose beta follows from theta; stepCount, the times, the mini-batch edges and the two
  // updaters' step counters are carried over, so the step size continues.  Its RNG streams, sampler state (the pending
  // mini-batch included) and perplexity running mean are its own fresh ones.  This learner is only drained.  Both pi
  // matrices are alive at once.  Throws std::invalid_argument on a bad map (the id is named) and when the run is sharded.
  std::unique_ptr<Learner> Reduce(const std::vector<int32_t>& map);
  uint64_t ReducedFromK() const { return reduced_from_K_; }  // 0: not made by Reduce
  uint64_t EmptiedRows() const { return emptied_rows_; }     // rows the plan left without mass (set uniform)
  std::vector<Float> GetPhiSum();

  // Reading the model out (include/ammsb_readout.h; not in the reference API).  Per node its `top` (1..16) strongest
  // communities, value descending and equal values by community ascending: ids / weights are [N, top], a slot below
  // `threshold` (>= 0) or past K holds 0xFFFFFFFF / 0; count[a] = communities >= threshold, not capped at top;
  // sizes[k] = nodes with pi[a, k] >= threshold.  Any of the four may be nullptr.  Waits for the work in flight as
  // Serialize does, reads this rank's pi (every rank holds all of it: not a collective) in row slabs of bounded
  // output, and touches nothing of the iteration.  Throws std::invalid_argument on a bad top / threshold.
  void Memberships(uint32_t top, Float threshold, std::vector<uint32_t>* ids, std::vector<Float>* weights,
                   std::vector<uint32_t>* count, std::vector<uint64_t>* sizes);
  // ... and as communities: members of community k = members[offsets[k] .. offsets[k + 1]), ascending node ids; a
  // node is a member of the communities in its non-empty Memberships slots.  sizes as above (may be nullptr).
  void Communities(uint32_t top, Float threshold, std::vector<uint64_t>* offsets, std::vector<uint32_t>* members,
                   std::vector<uint64_t>* sizes);
  // `# N K top threshold`, then one line `k size n0 n1 ...` per community.
  bool WriteCommunities(std::ostream* out, uint32_t top, Float threshold);

  // Predicting links (include/ammsb_linkpred.h; not in the reference API).  p(a, b) = eps + sum_k pi_ak pi_bk
  // (beta_k - eps) per edge key of `edges` (either order of the ends; -1 for an end >= N) ...
  void LinkProbabilities(const std::vector<Edge>& edges, std::vector<Float>* out);
  // ... and per node of `nodes` its `top` (1..64) most probable partners among all N nodes that are not the node itself
  // and whose pair is in none of the edge sets named by exclude_mask: ids / scores are [nodes.size(), top], score
  // descending and equal scores by id ascending, 0xFFFFFFFF / 0 in the slots past the eligible nodes.  Both wait for the
  // work in flight as Serialize does, read this rank's pi (not a collective), go in query slabs of bounded output, and
  // touch nothing of the iteration.  Throw std::invalid_argument on a bad top, mask or node id >= N.
  enum : uint32_t { kExcludeTraining = 1u, kExcludeHeldout = 2u };
  void PredictLinks(const std::vector<Vertex>& nodes, uint32_t top, uint32_t exclude_mask, std::vector<Vertex>* ids,
                    std::vector<Float>* scores);
  // `# N K top exclude` (exclude: none | training | heldout | all), then one line `a n b0 s0 b1 s1 ...` per query node
  // (n = its non-empty slots); scores printed with %.9g, so they parse back to the same binary32.
  bool WritePredictedLinks(std::ostream* out, const std::vector<Vertex>& nodes, uint32_t top, uint32_t exclude_mask);

  // The communities that explain a link (include/ammsb_linkcomm.h; not in the reference API).  Per edge key of `edges`
  // (either order of the ends) the `top` (1..16) largest terms t_k = (pi_ak pi_bk) beta_k that are > 0 and >= min_term,
  // with their communities: ids / terms are [edges.size(), top], term descending and equal terms by community
  // ascending, 0xFFFFFFFF / 0 in the empty slots; prob is p(a, b) as LinkProbabilities defines it (-1 and empty slots
  // for an end >= N).  Terms are exact binary32 products; t_k / p is the posterior that the link is a community-k link.
  // Waits for the work in flight as Serialize does, reads this rank's pi (not a collective), goes in slabs of bounded
  // output, and touches nothing of the iteration.  Throws std::invalid_argument on a bad top or min_term.
  void LinkCommunities(const std::vector<Edge>& edges, uint32_t top, Float min_term, std::vector<uint32_t>* ids,
                       std::vector<Float>* terms, std::vector<Float>* prob);
  // sizes: [K + 1], per community the training links whose largest term it holds; sizes[K] = the training links no
  // community explains at min_term.  One pass that writes nothing else.
  void LinkCommunitySizes(Float min_term, std::vector<uint64_t>* sizes);
  // `# N K E top min_term`, then one line `a b p n k0 t0 k1 t1 ...` per training link in ascending key order (n = its
  // filled slots); floats printed with %.9g, so they parse back to the same binary32.
  bool WriteLinkCommunities(std::ostream* out, uint32_t top, Float min_term);

  // Scoring communities against the graph (include/ammsb_quality.h; not in the reference API).  Node a is a member of
  // community k iff pi[a, k] >= threshold (a binary32 compare).  Over the training links: size [K] = the members of k (as
  // Memberships' sizes), internal [K] = the links with both ends in k, boundary [K] = the links with exactly one end in
  // k, uncovered = the links whose ends share no community.  Exact counts.  Waits for the work in flight as Serialize
  // does, reads this rank's pi (not a collective), and touches nothing of the iteration.  Throws std::invalid_argument
  // on a threshold that is negative, NaN or infinite.
  void CommunityQuality(Float threshold, std::vector<uint64_t>* size, std::vector<uint64_t>* internal,
                        std::vector<uint64_t>* boundary, uint64_t* uncovered);
  // `# N K E threshold uncovered`, then one line `k size internal boundary conductance density` per community, the
  // derived measures as include/ammsb_quality.h defines them (-1 where undefined); floats printed with %.9g.
  bool WriteCommunityQuality(std::ostream* out, Float threshold);

  // Matching the detected cover to a ground-truth cover (include/ammsb_cover.h; not in the reference API).  The detected
  // community k is {a : pi[a, k] >= threshold} (a binary32 compare); the ground truth is a CSR, offsets [G + 1] ascending
  // from 0 to members.size(), taken as written (a duplicate counts twice; a member >= N reads nothing and is counted
  // in `skipped`).  Per ground-truth community the detected community of the best F1 = 2 overlap / (t_g + d_k) among
  // those it overlaps (equal -> the lower k, none -> -1), the overlap and t_g; the same per detected community over the
  // ground-truth ones; detected_size = the members of every detected community among all N nodes.  Exact integers.
  // `overlap`, if not null, receives the dense [G, K] matrix.  Waits for the work in flight as Serialize does, reads
  // this rank's pi (not a collective), and touches nothing of the iteration.  Throws std::invalid_argument on a
  // threshold that is negative, NaN or infinite and on offsets that do not describe `members`.
  struct CoverMatch {
    std::vector<int32_t> truth_best, detected_best;
    std::vector<uint32_t> truth_overlap, truth_size, detected_overlap;
    std::vector<uint64_t> detected_size;
    uint64_t skipped = 0;
    // float64, as include/ammsb_cover.h states the measures: the F1 of every best match (0 for none) and the means
    // over the non-empty communities (-1 where a mean is over nothing); filled by Derive()
    std::vector<double> f1_truth_each, f1_detected_each;
    double f1_truth = -1, f1_detected = -1, avg_f1 = -1;
    void Derive();
  };
  void CompareCover(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, Float threshold,
                    CoverMatch* match, std::vector<uint32_t>* overlap = nullptr);
  // `# N K G threshold skipped f1_truth f1_detected avg_f1`, then the G lines `t g size best overlap f1` and the K
  // lines `d k size best overlap f1`; floats printed with %.9g.
  bool WriteCoverMatch(std::ostream* out, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members,
                       Float threshold);

  // The overlapping NMI of the detected cover against the same kind of ground truth (include/ammsb_nmi.h): the dense
  // overlap is made slab by slab (Gs communities with Gs K 4 <= slab_bytes, Gs >= 1) by the cover match and folded on
  // the device into one minimum per community; every float comes from the device, the host applies the fallback
  // h = min(c, H) and adds in index order.  NMI is defined on sets: std::invalid_argument on a community that lists a
  // node twice, besides what CompareCover throws.  Waits, reads and perturbs like CompareCover.
  struct CoverNmi {
    std::vector<uint32_t> truth_size;
    std::vector<uint64_t> detected_size;
    uint64_t skipped = 0;
    std::vector<double> H_truth, H_detected;  // H(X_g), H(Y_k)
    std::vector<double> h_truth, h_detected;  // H(X_g | Y), H(Y_k | X)
    double nmi_lfk = -1, nmi_max = -1;        // -1 where undefined
    void Derive();                            // the two scores from the four arrays
  };
  void CoverNMI(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, Float threshold,
                CoverNmi* nmi, uint64_t slab_bytes = 256ull << 20);
  // `# N K G threshold skipped nmi_lfk nmi_max`, then the G lines `t g size H h` and the K lines `d k size H h`;
  // floats printed with %.17g.
  bool WriteCoverNMI(std::ostream* out, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members,
                     Float threshold, uint64_t slab_bytes = 256ull << 20);

  // The Omega index (Collins & Dent) of the detected cover against the same kind of ground truth over the pairs of a
  // universe of nodes (include/ammsb_omega.h): `universe` holds ascending, distinct ids < N (OmegaUniverse makes the two
  // standard ones).  Integer counts from the device; the score in signed 128-bit integers, their quotient rounded to
  // double once.  std::invalid_argument on a bad threshold, CSR or universe and on a community
  // that lists a node twice; std::runtime_error past 65536 ground-truth communities or 4095 memberships of one node.
  // Waits, reads and perturbs like CompareCover.
  struct OmegaIndex {
    uint64_t nodes = 0, skipped = 0, outside = 0;
    std::vector<uint64_t> agree, detected, truth;  // [L]: pairs by the communities they share
    double omega = 0, omega_unadjusted = 0;        // NaN where undefined (the index itself can be negative)
    void Derive();                                 // the two scores from the three histograms and `nodes`
  };
  // kind: "covered" (the nodes with at least one member entry < N) or "all"; std::invalid_argument otherwise
  static std::vector<uint32_t> OmegaUniverse(const std::string& kind, const std::vector<uint32_t>& members, uint64_t N);
  void CoverOmega(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, Float threshold,
                  const std::vector<uint32_t>& universe, OmegaIndex* omega, uint64_t launch_pairs = 1ull << 31);
  // `# N K G threshold universe_n skipped outside omega omega_unadjusted`, then the L lines `j agree detected truth`;
  // floats printed with %.17g, NaN as `nan`.
  bool WriteCoverOmega(std::ostream* out, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members,
                       Float threshold, const std::vector<uint32_t>& universe, uint64_t launch_pairs = 1ull << 31);

  // How the detected communities relate to each other (include/ammsb_relate.h).  CommunityOverlap: overlap[K * K], the
  // nodes a with pi[a, k] >= threshold and pi[a, l] >= threshold; symmetric, the diagonal holds the community sizes.  The
  // nodes are cut into slabs of a multiple of 64 rows whose membership bits, K rows / 8 bytes, fit max_bytes (at least
  // 64 rows); integer adds, so the result does not depend on max_bytes.  RelatedCommunities: per community the `top`
  // (1..64) others that share at least max(1, min_overlap) nodes with it, ranked by `by` -- "overlap" (the shared nodes
  // o), "jaccard" (o / (d_k + d_l - o)) or "contained" (o / d_l) -- as exact rationals, equal values by id ascending.
  // std::invalid_argument on a bad threshold, measure or top.  Waits, reads and perturbs like CommunityQuality.
  struct Related {
    std::vector<uint64_t> size;     // [K]
    std::vector<int32_t> partner;   // [K * top], -1 in an empty slot
    std::vector<uint32_t> overlap;  // [K * top], the nodes shared with that partner, 0 in an empty slot
  };
  void CommunityOverlap(Float threshold, std::vector<uint32_t>* overlap, uint64_t max_bytes = 1ull << 30);
  void RelatedCommunities(Float threshold, uint32_t top, const std::string& by, uint32_t min_overlap, Related* related,
                          uint64_t max_bytes = 1ull << 30);
  // `# N K threshold by top min_overlap`, then `k size n l0 o0 l1 o1 ...` per community: integers below the header.
  bool WriteRelatedCommunities(std::ostream* out, Float threshold, uint32_t top, const std::string& by,
                               uint32_t min_overlap = 1, uint64_t max_bytes = 1ull << 30);

  // How the detected communities are linked to each other (include/ammsb_connect.h), over the training links (every link
  // once as (min << 32) | max).  CommunityLinks: links[K * K] = directed + its transpose, directed[k, l] counting the
  // links (a, b) with pi[a, k] >= threshold and pi[b, l] >= threshold; symmetric, the diagonal is twice CommunityQuality's
  // internal.  LinkedCommunities: per community the `top` (1..64) others with at least max(1, min_links) links to it,
  // ranked by `by` -- "links" (the count w) or "density" (w over the d_k d_l - overlap[k, l] ordered pairs of distinct
  // nodes; no such pair: no partner) -- as exact rationals, equal values by id ascending; the overlap is
  // CommunityOverlap(threshold, max_bytes).  std::invalid_argument on a bad threshold, measure or top.  Waits, reads and
  // perturbs like CommunityQuality.
  struct Linked {
    std::vector<uint64_t> size;      // [K]
    std::vector<uint64_t> internal;  // [K], the links inside k
    std::vector<int32_t> partner;    // [K * top], -1 in an empty slot
    std::vector<uint64_t> links;     // [K * top], the links between k and that partner, 0 in an empty slot
    std::vector<uint32_t> shared;    // [K * top], the nodes shared with that partner, 0 in an empty slot
    uint64_t valid = 0, skipped = 0; // the training links counted; those with an end >= N (none)
  };
  void CommunityLinks(Float threshold, std::vector<uint64_t>* links);
  void LinkedCommunities(Float threshold, uint32_t top, const std::string& by, uint64_t min_links, Linked* linked,
                         uint64_t max_bytes = 1ull << 30);
  // `# N K E threshold by top min_links skipped`, then `k size internal n l0 w0 o0 l1 w1 o1 ...` per community: integers
  // below the header.
  bool WriteLinkedCommunities(std::ostream* out, Float threshold, uint32_t top, const std::string& by,
                              uint64_t min_links = 1, uint64_t max_bytes = 1ull << 30);

  // Is the cover better than chance?  The overlapping modularity (EQ of Shen et al.) of the cover pi[a, k] >= threshold
  // against `edges` (keys (a << 32) | b as include/ammsb_modularity.h takes them; nullptr: every training link once),
  // fewer than 2^31 keys.  internal and volume are the device's 128-bit sums IN and SV in units of 2^-62, exact; Derive()
  // is the header's float64 statement over them: one conversion that rounds once, ldexp, then q_k = (2 in_k - s_k s_k /
  // (2m)) / (2m) and q = the sum in index order, -1 when m = 0.  std::invalid_argument on a bad threshold or a list of
  // 2^31 keys or more.  Waits, reads and perturbs like CommunityQuality.
  struct ModularityScore {
    std::vector<unsigned __int128> internal, volume;  // [K]
    std::vector<uint32_t> degree;                     // [N]
    uint64_t links = 0, skipped = 0;                  // m, the valid keys; those with an end >= N
    double q = -1;
    std::vector<double> q_each, in_each, s_each;      // [K]
    void Derive();
  };
  void Modularity(Float threshold, const std::vector<Edge>* edges, ModularityScore* result);
  // `# N K E threshold skipped q`, then `k q_k in_k s_k internal volume` per community: %.17g and 32 hexadecimal digits.
  bool WriteModularity(std::ostream* out, Float threshold, const std::vector<Edge>* edges = nullptr);

  // How does a single node sit in the cover?  Per node of an adjacency (nullptr: the training graph's rows; else both
  // directions of every key (a << 32) | b of `edges`, a key with an end >= N counted in skipped) the integers of
  // include/ammsb_roles.h for the cover pi[a, k] >= threshold: with c[a, k] the neighbours of a in k, degree, own,
  // embedded, reached, votes, squares, the `top` (1..16) communities with the largest c (among "all": every k with c >=
  // max(1, min_count); "own": a's communities with c >= min_count) and per community ksum, ksq, kmembers, all exact.
  // Derive() is the header's float64 statement over them.  std::invalid_argument on a bad threshold, top or among, or a
  // row of more than 2^25 targets.  Waits, reads and perturbs like CommunityQuality.
  struct NodeRolesResult {
    uint32_t top = 0;
    std::vector<uint32_t> degree, own, embedded, reached, hflags;  // [N]
    std::vector<uint64_t> votes, squares;                          // [N]
    std::vector<int32_t> home;                                     // [N, top], -1: empty
    std::vector<uint32_t> hcount;                                  // [N, top]
    std::vector<uint64_t> ksum, ksq, kmembers;                     // [K]
    uint64_t valid = 0, skipped = 0;                               // targets counted; targets or keys with an end >= N
    std::vector<double> embeddedness, participation, z;            // [N], [N], [N, top]
    void Derive();
  };
  void NodeRoles(Float threshold, const std::vector<Edge>* edges, uint32_t top, const std::string& among, uint32_t min_count,
                 NodeRolesResult* result);
  // `# N K M threshold among top min_count skipped`, `c k members ksum ksq` per community, `n a degree own embedded reached
  // votes squares nslots k0 c0 f0 ...` per node: integers throughout.
  bool WriteNodeRoles(std::ostream* out, Float threshold, uint32_t top = 4, const std::string& among = "all",
                      uint32_t min_count = 0, const std::vector<Edge>* edges = nullptr);

  // Do the communities hold triangles?  Over the simple adjacency of `edges` (nullptr: every training link once; else the
  // keys (a << 32) | b: both directions of every key with both ends < N, each row sorted and made unique, loops removed; a
  // key with an end >= N counted in skipped, repeats and loops in dropped) the integers of include/ammsb_triangles.h for
  // the cover pi[a, k] >= threshold: per node degree, tri, tri_in, tri_comms, per community ktri3, kpart, and from one run
  // of the node roles without a selection over the same rows kmembers and wedges = (ksq - ksum) / 2, all exact.  Derive()
  // is the header's float64 statement over them.  std::invalid_argument on a bad threshold or a row of more than 65535
  // targets.  Waits, reads and perturbs like CommunityQuality.
  struct TrianglesResult {
    std::vector<uint32_t> degree, tri, tri_in, tri_comms;  // [N]
    std::vector<uint64_t> ktri3, kpart, kmembers, wedges;   // [K]
    uint64_t M = 0, skipped = 0, dropped = 0;               // targets of the simple adjacency; keys left out
    std::vector<double> tpr, clustering;                    // [K], -1 where not defined
    std::vector<uint64_t> triangles;                        // [K]
    std::vector<double> local_clustering, inside;           // [N], -1 where not defined
    uint64_t total = 0;
    double transitivity = -1, avg_clustering = -1;
    void Derive();  // std::logic_error where 3 does not divide a count over all nodes
  };
  void Triangles(Float threshold, const std::vector<Edge>* edges, TrianglesResult* result);
  // `# N K M threshold skipped dropped total`, `c k members part tri3 wedges` per community, `n a degree tri tri_in
  // tri_comms` per node: integers throughout.
  bool WriteTriangles(std::ostream* out, Float threshold, const std::vector<Edge>* edges = nullptr);

  // Is each community one piece?  The connected components of every community of the cover pi[a, k] >= threshold inside the
  // graph of `edges` (nullptr: every training link once; else the keys (a << 32) | b, either order of the ends, duplicates
  // and a == a valid, a key with an end >= N counted in skipped), the integers of include/ammsb_components.h: per community
  // members, components, largest, largest_root (-1: empty), singletons; the memberships as a CSR over the nodes, offsets
  // [N + 1] (a host prefix sum over the downloaded own) and per slot community, root (the smallest node of its component),
  // size; stray per node; links, skipped, shared, all exact.  Derive() is the header's float64 statement over them.
  // std::invalid_argument on a bad threshold, on a cover of 2^32 memberships or more (the message names the threshold) and
  // on a list of 2^31 keys or more; std::runtime_error where the library gave a union up.  Waits, reads and perturbs like
  // CommunityQuality.
  struct ComponentsResult {
    std::vector<uint64_t> members, components, singletons;  // [K]
    std::vector<uint32_t> largest;                           // [K]
    std::vector<int32_t> largest_root;                       // [K]
    std::vector<uint64_t> offsets;                           // [N + 1]
    std::vector<uint16_t> community;                         // [M]
    std::vector<uint32_t> root, size;                        // [M]
    std::vector<uint32_t> stray;                             // [N]
    uint64_t links = 0, skipped = 0, shared = 0;
    std::vector<double> giant, fragmentation;                // [K], -1 where members is 0
    double connected = -1;
    void Derive();
  };
  void CommunityComponents(Float threshold, ComponentsResult* result, const std::vector<Edge>* edges = nullptr);
  // `# N K E M threshold skipped shared`, `c k members components largest largest_root singletons` per community, `n a
  // nslots k0 root0 size0 ...` per node: integers throughout.
  bool WriteCommunityComponents(std::ostream* out, Float threshold, const std::vector<Edge>* edges = nullptr);

  // Where does a node sit inside a community?  The k-core decomposition of the subgraph every community of the cover pi[a,
  // k] >= threshold induces in the simple adjacency of `edges` (as Triangles builds it on the host, without its limit on a
  // row's length; nullptr: every training link once), the integers of include/ammsb_cores.h: per community members,
  // inlinks2, degeneracy, nucleus, isolated; the memberships as a CSR over the nodes, offsets [N + 1] and per slot
  // community, indeg, core; best_core, best_comm (-1: no community), in_nucleus per node; L, skipped, dropped, all exact,
  // and the launch counts scans and rounds (diagnostic).  Derive() is the header's float64 statement over them.
  // std::invalid_argument on a bad threshold, on a cover of 2^32 memberships or more and on neighbour lists of 2^32
  // entries or more than max_bytes (both messages name the threshold).  Waits, reads and perturbs like CommunityQuality.
  struct CoresResult {
    std::vector<uint64_t> members, inlinks2, nucleus, isolated;  // [K]
    std::vector<uint32_t> degeneracy;                             // [K]
    std::vector<uint64_t> offsets;                                // [N + 1]
    std::vector<uint16_t> community;                              // [M]
    std::vector<uint32_t> indeg, core;                            // [M]
    std::vector<uint32_t> best_core, in_nucleus;                  // [N]
    std::vector<int32_t> best_comm;                               // [N]
    uint64_t L = 0, skipped = 0, dropped = 0, scans = 0, rounds = 0;
    std::vector<double> coreness;                                 // [M], -1 where the degeneracy is 0
    std::vector<double> nucleus_share, mean_core;                 // [K], -1 where members is 0
    void Derive();
  };
  void CommunityCores(Float threshold, CoresResult* result, const std::vector<Edge>* edges = nullptr,
                      uint64_t max_bytes = 4ull << 30);
  // `# N K M L threshold skipped dropped`, `c k members inlinks2 degeneracy nucleus isolated` per community, `n a nslots k0
  // indeg0 core0 ...` per node: integers throughout.
  bool WriteCommunityCores(std::ostream* out, Float threshold, const std::vector<Edge>* edges = nullptr);

 private:
  Float DoSample(Sample* sample);        // learner.cc:175-194
  Float DoSampleDevice(Sample* sample);  // Config::device_sampling: csrc/ammsb_minibatch.hip instead of sample.cc
  Float DoSampleReference(Sample* sample);  // ... with sampling_stream "reference": csrc/ammsb_refsample.hip
  bool SerializeDeviceSampler(std::ostream* out);
  void RunAsync(uint32_t max_iters, sig_atomic_t* signaled);  // Config::async_launch + device_sampling
  void RunGraph(uint32_t max_iters, sig_atomic_t* signaled);  // Config::graph_launch: iterations as captured graphs
  void AccountLoopStamps(uint32_t first_step, uint32_t n_steps);  // in-kernel time stamps -> PrintStats categories
  ammsb_mb_choice ChooseDevice();                             // the next mini-batch: (link?, u, deg(u), candidates)
  Float EnqueueDevice(Sample* sample, const ammsb_mb_choice& choice);
  void DrainAsync();
  bool ParseDeviceSampler(std::istream* in);
  uint32_t CandidatesFor(uint64_t u);  // candidate draws of a non-link mini-batch of vertex u
  uint32_t CandidatesForExcluded(uint32_t excluded);
  void CheckDeviceSampler();           // throws if a mini-batch came up short since the last check
  // multi-GPU (Config::exchange with world() > 1; new, see include/mcmc/exchange.h): every rank runs the same
  // learner on the same data and seeds, computes its block of update_phi's virtual groups / its slice of the
  // gradient's and the perplexity's edges, and exchanges phi_vec rows, [2K] gradient partials and the 4 sums.
  bool Sharded() const;
  void Step(Sample& s, Float weight);  // phi, pi, beta of one iteration (sharded or not)
  void StepSharded(Sample& s, Float weight);
  Float Perplexity(PerplexityCalculator* calc);
  void GatherShardedState();  // before a checkpoint: owners hand out their phi streams and running means
  // The (pi, beta) a post-fit method reads, called after it has drained the loop: the last draw, or under ReadAverage(true)
  // the mean with every row flushed (host/postfit.cc)
  const ammsb_rpm& PostfitPi();
  const Float* PostfitBeta();
  void FlushAverage();  // every row of mean_pi_ and mean_beta_ up to avg_n_; nothing is launched when nothing ran since
  void FlushRows(const uint32_t* nodes, uint64_t first, uint64_t count);  // through the library the average was started with
  void NeedSpread(const char* what) const;
  const ammsb_rpm& BoundPi();

  std::unique_ptr<Config> owned_cfg_;  // a learner made by Reduce(): what cfg_ refers to (first member: destroyed last)
  uint64_t reduced_from_K_ = 0, emptied_rows_ = 0;
  const Config& cfg_;
  clcuda::Queue queue_;
  clcuda::Buffer<Float> beta_;
  clcuda::Buffer<Float> theta_;
  std::shared_ptr<RowPartitionedMatrixFactory<Float>> allocFactory_;
  std::unique_ptr<RowPartitionedMatrix<Float>> pi_;
  clcuda::Buffer<Float> phi_;
  std::shared_ptr<OpenClSetFactory> setFactory_;
  std::unique_ptr<OpenClSet> trainingSet_;
  std::unique_ptr<OpenClSet> heldoutSet_;
  clcuda::Buffer<Edge> heldoutEdges_;
  // Config::calc_train_ppx (the reference's MCMC_CALC_TRAIN_PPX members, learner.h:65-69)
  std::vector<Edge> trainingPerplexityEdges_;
  std::unique_ptr<clcuda::Buffer<Edge>> devTrainingPerplexityEdges_;
  std::unique_ptr<PerplexityCalculator> trainingPerplexity_;
  PerplexityCalculator heldoutPerplexity_;
  PhiUpdater phiUpdater_;
  BetaUpdater betaUpdater_;
  SamplerFn sampler_;
  uint32_t stepCount_;
  uint64_t time_, samplingTime_, edges_done_;
  // device sampler state (only with Config::device_sampling)
  std::shared_ptr<ammsb_ctx> ctx_;
  std::unique_ptr<clcuda::Buffer<uint64_t>> csr_offsets_;
  std::unique_ptr<clcuda::Buffer<Vertex>> csr_targets_;
  std::vector<uint32_t> degree_;
  std::vector<uint32_t> excluded_;  // 1 + training degree + held-out link degree
  std::map<uint32_t, uint32_t> cand_cache_;
  uint32_t candidates_ = 0;
  std::unique_ptr<random::OpenClRandom> mb_rand_;
  std::unique_ptr<clcuda::Buffer<uint8_t>> mb_workspace_;
  std::unique_ptr<clcuda::Buffer<uint32_t>> mb_count_;
  std::mt19937_64 host_rng_;
  // Config::sampling_stream == "reference": the reference's rand_r stream on the device (libammsb_refsample.so)
  bool ref_stream_ = false;
  void* ref_ = nullptr;  // ammsb_refsample*
  // async loop: per sample, `ready` (sampling done, recorded on the sample's stream) and `consumed` (the
  // iteration that used it is done, recorded on the main stream); weights of the enqueued samples
  void* ev_ready_[2] = {nullptr, nullptr};
  void* ev_consumed_[2] = {nullptr, nullptr};
  bool consumed_valid_[2] = {false, false};
  void* ev_sampler_ = nullptr;  // the device sampler's shared streams / workspace: one call at a time
  bool sampler_valid_ = false;
  uint32_t chunks_since_check_ = 0;  // RunGraph: chunks enqueued since the last ammsb_loop_check
  bool enqueued_[2] = {false, false};
  Float weights_[2] = {0, 0};
  ammsb_mb_choice choice_[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};  // what sits in each sample's buffers (device sampling)
  ammsb_loop* loop_ = nullptr;
  // Ownership map of the sharded update_phi: groups [0, g_rep_) are replicated (every rank computes them); the rest are
  // cut into world * nch_ blocks of cc_ groups, block b owned by rank b % world and exchanged in chunk b / world.
  uint32_t cc_ = 0, g_rep_ = 0, nch_ = 1;
  void SetSplit(uint32_t g_rep);
  void CalibrateSplit();              // Config::phi_replicate < 0: balance recomputing a group against receiving it
  void PlacePi();                     // Config::pi_placement_candidates: keep the allocation of pi update_phi runs fastest over
  void* xstream_ = nullptr;           // the exchanges of a step run here, beside the next block's update_phi
  void* ev_block_ = nullptr;          // main stream: a block's update_phi has been enqueued (the exchange waits for it)
  void* ev_xdone_ = nullptr;          // exchange stream: the step's exchanges are done (the main stream waits for it)
  double calib_phi_ms_ = 0, calib_xchg_ms_ = 0;
  std::unique_ptr<clcuda::Buffer<Float>> all_grads_, grads_sum_, tail_buf_;
  std::unique_ptr<clcuda::Buffer<ammsb_ppx_sums>> all_sums_;
  // the chain average: mean_pi_[a, :] is the mean of the samples 1 .. avg_last_[a], and the samples after that equal pi
  bool averaging_ = false, read_average_ = false;
  uint32_t avg_n_ = 0, avg_flushed_ = 0;
  std::unique_ptr<RowPartitionedMatrix<Float>> mean_pi_;
  std::unique_ptr<clcuda::Buffer<uint32_t>> avg_last_;
  std::unique_ptr<clcuda::Buffer<double>> mean_beta64_;
  std::unique_ptr<clcuda::Buffer<Float>> mean_beta_;
  // ... and its spread: var_pi_ the population variance of the same samples, beta_m2_ Welford's sum for beta, bound_pi_ the
  // bound matrix ReadBound asked for, filled for bound_n_ samples at bound_filled_z_
  bool spread_ = false, read_bound_ = false;
  Float bound_z_ = -2, bound_filled_z_ = -2;
  uint32_t bound_n_ = 0;
  std::unique_ptr<RowPartitionedMatrix<Float>> var_pi_, bound_pi_;
  std::unique_ptr<clcuda::Buffer<double>> beta_m2_;
  std::unique_ptr<Sample> samples_[2];  // MCMC_SAMPLE_PARALLEL (CMakeLists.txt:42, default ON)
  std::future<Float> futures_[2];
  int phase_;
};

// learner.cc:47-75: the first training_ppx_ratio * |training| training edges, then links * (N(N-1)/2) / E random
// pairs (u != v, MakeEdge(u, v) as drawn -- NOT canonicalised, as in the reference) that are in neither set.
std::vector<Edge> MakeEdgesForTrainingPerplexity(const Config& cfg);

// A plan (the map of Learner::Reduce) as text, byte for byte what mcmc-ammsb-gpu_amd/_reduce.py writes: `# K new_K dropped`,
// then `j n k0 k1 ...` per new community (sources ascending) and `x k` per dropped one.  PlanSources validates a map and
// returns its inverse CSR (std::invalid_argument names the offending id); ReadPlan throws it for a file that is no plan.
void PlanSources(const std::vector<int32_t>& map, std::vector<uint32_t>* src_off, std::vector<uint32_t>* src);
bool WritePlan(std::ostream* out, const std::vector<int32_t>& map);
std::vector<int32_t> ReadPlan(std::istream* in);

}  // namespace mcmc

#endif  // MCMC_AMD_LEARNER_H_
