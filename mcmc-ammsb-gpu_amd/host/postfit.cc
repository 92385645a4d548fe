// mcmc::Learner's post-fit analyses (include/mcmc/learner.h): what reads a fitted model out -- memberships and
// communities, link prediction, link communities, community quality, the three comparisons with a ground-truth cover
// (F1 match, overlapping NMI, Omega index), how the detected communities relate to each other, how they are linked, the
// overlapping modularity of the cover, the role of every node in it, the triangles inside the communities and the connected
// components of each.  Each is
// a thin driver of one library of its own (libammsb_readout.so ... libammsb_components.so): check the arguments, drain the training loop, run the library in slabs of a fixed byte budget,
// read the results back, and for the Write* methods print them.  Nothing here touches the training loop of learner.cc.
#include "mcmc/learner.h"
#include "ammsb_readout.h"
#include "ammsb_linkpred.h"
#include "ammsb_linkcomm.h"
#include "ammsb_quality.h"
#include "ammsb_cover.h"
#include "ammsb_nmi.h"
#include "ammsb_omega.h"
#include "ammsb_relate.h"
#include "ammsb_connect.h"
#include "ammsb_modularity.h"
#include "ammsb_roles.h"
#include "ammsb_triangles.h"
#include "ammsb_components.h"
#include "ammsb_cores.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

namespace mcmc {

namespace {
// what a failed call of one of the post-fit libraries throws: its return code in words and the library's own detail
std::runtime_error PostfitError(const char* call, int rc, const char* detail) {
  return std::runtime_error(std::string(call) + ": " + ammsb_strerror(rc) + " (" + detail + ")");
}

// the membership threshold of the analyses that compare pi with it on the device (Memberships has a looser rule)
void CheckThreshold(const char* who, Float threshold) {
  if (!(threshold >= 0 && std::isfinite(threshold)))
    throw std::invalid_argument(std::string(who) + ": the threshold must be finite and >= 0");
}

// a ground-truth cover as (offsets, members): G + 1 ascending offsets into the member list, within the libraries' ranges
void CheckTruthCover(const char* who, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members) {
  if (offsets.empty() || offsets.front() != 0 || offsets.back() != members.size() ||
      !std::is_sorted(offsets.begin(), offsets.end()))
    throw std::invalid_argument(std::string(who) + ": offsets must ascend from 0 to the number of members");
  if (((offsets.size() - 1) >> 31) || (static_cast<uint64_t>(members.size()) >> 32))
    throw std::invalid_argument(std::string(who) + ": 2^31 communities or 2^32 members, or more");
}

// no ground-truth community lists a node twice; `what` is the measure that is defined on sets
void CheckSets(const char* who, const char* what, const std::vector<uint64_t>& offsets,
               const std::vector<uint32_t>& members) {
  std::vector<uint32_t> sorted;
  for (size_t g = 0; g + 1 < offsets.size(); ++g) {
    sorted.assign(members.begin() + offsets[g], members.begin() + offsets[g + 1]);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      throw std::invalid_argument(std::string(who) + ": ground-truth community " + std::to_string(g) +
                                  " lists a node twice (" + what + " is defined on sets)");
  }
}

// a number as the output files hold it: %.9g for what is a float, %.17g for what is a double, "nan" without a sign
std::string Num(double x, int digits) {
  if (x != x) return "nan";
  char buf[40];
  snprintf(buf, sizeof(buf), "%.*g", digits, x);
  return buf;
}
std::string G9(double x) { return Num(x, 9); }
std::string G17(double x) { return Num(x, 17); }

// bytes of device memory set to zero on the stream, for the analysis `who`
void Zero(const char* who, void* p, uint64_t bytes, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, stream);
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": memset: " + hipGetErrorString(e));
}

// The node-major membership bits pi[a, k] >= threshold (libammsb_connect.so's mask) in a buffer of their own, filled on
// the stream; a failure is reported under the name `call`.  fill = false only allocates (a buffer needs a byte).
clcuda::Buffer<uint64_t> MembershipMask(const char* call, const ammsb_rpm* pi, Float threshold,
                                        const clcuda::Context& context, hipStream_t stream, bool fill = true) {
  const uint64_t words = ammsb_connect_mask_bytes(pi->num_rows, static_cast<uint32_t>(pi->num_cols)) / sizeof(uint64_t);
  clcuda::Buffer<uint64_t> d_mask(context, std::max<uint64_t>(words, 1));
  if (fill) {
    const int rc = ammsb_connect_mask(pi, threshold, d_mask(), stream);
    if (rc != AMMSB_OK) throw PostfitError(call, rc, ammsb_connect_last_error());
  }
  return d_mask;
}
}  // namespace

// ---- what the analyses read: the last draw, or under ReadAverage(true) the chain average with every row flushed -- with
// ReadBound(true, z) as well, the credible bound clamp(mean + z sd, 0, 1) of pi beside the mean of beta.  Every
// method calls these after it has drained the loop, so the flush is enqueued behind the last iteration.
const ammsb_rpm& Learner::PostfitPi() {
  if (!read_average_) return pi_->Get();
  if (read_bound_) return BoundPi();
  FlushAverage();
  return mean_pi_->Get();
}

const Float* Learner::PostfitBeta() {
  if (!read_average_) return beta_.data();
  FlushAverage();
  return mean_beta_->data();
}

// ---- reading the model out: libammsb_readout.so over pi, in row slabs whose outputs stay under a fixed byte budget
void Learner::Memberships(uint32_t top, Float threshold, std::vector<uint32_t>* ids, std::vector<Float>* weights,
                          std::vector<uint32_t>* count, std::vector<uint64_t>* sizes) {
  if (top == 0 || top > AMMSB_READOUT_MAX_TOP) throw std::invalid_argument("Memberships: top must be in 1..16");
  if (!(threshold >= 0)) throw std::invalid_argument("Memberships: the threshold must be >= 0");
  DrainAsync();
  queue_.Finish();
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  const bool tops = ids || weights || count;
  const uint64_t slab = std::min<uint64_t>(std::max<uint64_t>(N, 1), (64ull << 20) / (8ull * top + 4));
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<uint32_t> d_ids(context, tops ? slab * top : 1), d_count(context, tops ? slab : 1);
  clcuda::Buffer<Float> d_weights(context, tops ? slab * top : 1);
  std::unique_ptr<clcuda::Buffer<uint64_t>> d_sizes;
  if (sizes) {
    sizes->assign(K, 0);
    d_sizes.reset(new clcuda::Buffer<uint64_t>(context, queue_, sizes->begin(), sizes->end()));
  }
  if (ids) ids->resize(N * top);
  if (weights) weights->resize(N * top);
  if (count) count->resize(N);
  for (uint64_t lo = 0; lo < N; lo += slab) {
    const uint64_t n = std::min(slab, N - lo);
    const int rc = ammsb_readout_top(&PostfitPi(), nullptr, lo, n, top, threshold, tops ? d_ids() : nullptr,
                                     tops ? d_weights() : nullptr, tops ? d_count() : nullptr,
                                     d_sizes ? (*d_sizes)() : nullptr, queue_.stream());
    if (rc != AMMSB_OK)
      throw PostfitError("ammsb_readout_top", rc, ammsb_readout_last_error());
    if (ids) d_ids.Read(queue_, n * top, ids->data() + lo * top);
    if (weights) d_weights.Read(queue_, n * top, weights->data() + lo * top);
    if (count) d_count.Read(queue_, n, count->data() + lo);
  }
  if (sizes) d_sizes->Read(queue_, K, sizes->data());
  queue_.Finish();
}

void Learner::Communities(uint32_t top, Float threshold, std::vector<uint64_t>* offsets, std::vector<uint32_t>* members,
                          std::vector<uint64_t>* sizes) {
  std::vector<uint32_t> ids;
  Memberships(top, threshold, &ids, nullptr, nullptr, sizes);
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  offsets->assign(K + 1, 0);
  for (uint32_t id : ids)
    if (id != AMMSB_READOUT_NONE) ++(*offsets)[id + 1];
  for (uint64_t k = 0; k < K; ++k) (*offsets)[k + 1] += (*offsets)[k];
  members->assign((*offsets)[K], 0);
  std::vector<uint64_t> fill(offsets->begin(), offsets->end() - 1);
  for (uint64_t a = 0; a < N; ++a)  // ascending nodes, so every community's list comes out ascending
    for (uint32_t t = 0; t < top; ++t) {
      const uint32_t id = ids[a * top + t];
      if (id != AMMSB_READOUT_NONE) (*members)[fill[id]++] = static_cast<uint32_t>(a);
    }
}

bool Learner::WriteCommunities(std::ostream* out, uint32_t top, Float threshold) {
  std::vector<uint64_t> offsets, sizes;
  std::vector<uint32_t> members;
  Communities(top, threshold, &offsets, &members, &sizes);
  const uint64_t K = pi_->Cols();
  *out << "# " << pi_->Rows() << " " << K << " " << top << " " << G9(threshold) << "\n";
  for (uint64_t k = 0; k < K; ++k) {
    *out << k << " " << sizes[k];
    for (uint64_t i = offsets[k]; i < offsets[k + 1]; ++i) *out << " " << members[i];
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- predicting links: libammsb_linkpred.so over (pi, beta), eps as the kernels hold it (MakeKernelParams)
void Learner::LinkProbabilities(const std::vector<Edge>& edges, std::vector<Float>* out) {
  DrainAsync();
  queue_.Finish();
  out->assign(edges.size(), 0);
  if (edges.empty()) return;
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<Edge> d_edges(context, queue_, edges.begin(), edges.end());
  clcuda::Buffer<Float> d_out(context, edges.size());
  const int rc = ammsb_linkpred_pairs(&PostfitPi(), PostfitBeta(), MakeKernelParams(cfg_).epsilon, d_edges(), edges.size(),
                                      d_out(), queue_.stream());
  if (rc != AMMSB_OK)
    throw PostfitError("ammsb_linkpred_pairs", rc, ammsb_linkpred_last_error());
  d_out.Read(queue_, edges.size(), out->data());
  queue_.Finish();
}

void Learner::PredictLinks(const std::vector<Vertex>& nodes, uint32_t top, uint32_t exclude_mask,
                           std::vector<Vertex>* ids, std::vector<Float>* scores) {
  if (top == 0 || top > AMMSB_LINKPRED_MAX_TOP) throw std::invalid_argument("PredictLinks: top must be in 1..64");
  if (exclude_mask & ~(kExcludeTraining | kExcludeHeldout)) throw std::invalid_argument("PredictLinks: unknown exclude bits");
  const uint64_t N = pi_->Rows(), K = pi_->Cols(), Q = nodes.size();
  for (Vertex v : nodes)
    if (v >= N) throw std::invalid_argument("PredictLinks: a node id >= N");
  DrainAsync();
  queue_.Finish();
  ids->assign(Q * top, AMMSB_LINKPRED_NONE);
  scores->assign(Q * top, 0);
  if (Q == 0) return;
  const ammsb_set* ex[2] = {nullptr, nullptr};
  int n_ex = 0;
  if (exclude_mask & kExcludeTraining) ex[n_ex++] = &trainingSet_->Get();
  if ((exclude_mask & kExcludeHeldout) && heldoutSet_) ex[n_ex++] = &heldoutSet_->Get();
  // whole tiles of 128 queries whose outputs stay under a fixed byte budget; the workspace does not grow with Q
  const uint64_t slab = std::min<uint64_t>(Q, std::max<uint64_t>(128, (64ull << 20) / (8ull * top) / 128 * 128));
  const uint64_t ws_bytes = ammsb_linkpred_top_workspace_bytes(static_cast<uint32_t>(slab), top, N, K);
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<Vertex> d_nodes(context, queue_, nodes.begin(), nodes.end()), d_ids(context, slab * top);
  clcuda::Buffer<Float> d_scores(context, slab * top);
  clcuda::Buffer<uint64_t> d_ws(context, (ws_bytes + 7) / 8);
  const Float eps = MakeKernelParams(cfg_).epsilon;
  for (uint64_t lo = 0; lo < Q; lo += slab) {
    const uint64_t n = std::min(slab, Q - lo);
    const int rc = ammsb_linkpred_top(&PostfitPi(), PostfitBeta(), eps, d_nodes() + lo, static_cast<uint32_t>(n), top, ex[0],
                                      ex[1], 0, N, d_ids(), d_scores(), d_ws(), ws_bytes, queue_.stream());
    if (rc != AMMSB_OK)
      throw PostfitError("ammsb_linkpred_top", rc, ammsb_linkpred_last_error());
    d_ids.Read(queue_, n * top, ids->data() + lo * top);
    d_scores.Read(queue_, n * top, scores->data() + lo * top);
  }
  queue_.Finish();
}

bool Learner::WritePredictedLinks(std::ostream* out, const std::vector<Vertex>& nodes, uint32_t top,
                                  uint32_t exclude_mask) {
  std::vector<Vertex> ids;
  std::vector<Float> scores;
  PredictLinks(nodes, top, exclude_mask, &ids, &scores);
  static const char* const kNames[4] = {"none", "training", "heldout", "all"};
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << top << " " << kNames[exclude_mask & 3u] << "\n";
  for (size_t i = 0; i < nodes.size(); ++i) {
    uint32_t n = 0;
    while (n < top && ids[i * top + n] != AMMSB_LINKPRED_NONE) ++n;
    *out << nodes[i] << " " << n;
    for (uint32_t t = 0; t < n; ++t) *out << " " << ids[i * top + t] << " " << G9(scores[i * top + t]);
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- the communities that explain a link: libammsb_linkcomm.so over (pi, beta), eps as the kernels hold it
namespace {
void CheckLinkCommArgs(const char* who, uint32_t top, Float min_term) {
  if (top == 0 || top > AMMSB_LINKCOMM_MAX_TOP) throw std::invalid_argument(std::string(who) + ": top must be in 1..16");
  if (!(min_term >= 0 && std::isfinite(min_term)))
    throw std::invalid_argument(std::string(who) + ": min_term must be finite and >= 0");
}

// every training link once, ascending ((min << 32) | max is how an Edge is stored)
std::vector<Edge> SortedTrainingLinks(const Config& cfg) {
  std::vector<Edge> links(cfg.training_edges.begin(), cfg.training_edges.end());
  std::sort(links.begin(), links.end());
  links.erase(std::unique(links.begin(), links.end()), links.end());
  return links;
}

// The edge list an analysis runs over: the caller's, or where it passes none every training link, kept in *training and
// refused in the analysis's own name from `limit` of them on.
const std::vector<Edge>* EdgesOrTraining(const char* who, const std::vector<Edge>* edges, const Config& cfg,
                                         std::vector<Edge>* training, uint64_t limit = ~uint64_t(0)) {
  if (edges) return edges;
  *training = SortedTrainingLinks(cfg);
  if (training->size() >= limit) throw std::invalid_argument(std::string(who) + ": 2^31 training links or more");
  return training;
}
}  // namespace

void Learner::LinkCommunities(const std::vector<Edge>& edges, uint32_t top, Float min_term, std::vector<uint32_t>* ids,
                              std::vector<Float>* terms, std::vector<Float>* prob) {
  CheckLinkCommArgs("LinkCommunities", top, min_term);
  DrainAsync();
  queue_.Finish();
  const uint64_t n_all = edges.size();
  ids->assign(n_all * top, AMMSB_LINKCOMM_NONE);
  terms->assign(n_all * top, 0);
  prob->assign(n_all, 0);
  if (n_all == 0) return;
  const uint64_t slab = std::min<uint64_t>(n_all, std::max<uint64_t>(1, (64ull << 20) / (8ull * top + 4)));
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<Edge> d_edges(context, queue_, edges.begin(), edges.end());
  clcuda::Buffer<uint32_t> d_ids(context, slab * top);
  clcuda::Buffer<Float> d_terms(context, slab * top), d_prob(context, slab);
  const Float eps = MakeKernelParams(cfg_).epsilon;
  for (uint64_t lo = 0; lo < n_all; lo += slab) {
    const uint64_t n = std::min(slab, n_all - lo);
    const int rc = ammsb_linkcomm_edges(&PostfitPi(), PostfitBeta(), eps, d_edges() + lo, n, top, min_term, d_ids(),
                                        d_terms(), d_prob(), nullptr, queue_.stream());
    if (rc != AMMSB_OK)
      throw PostfitError("ammsb_linkcomm_edges", rc, ammsb_linkcomm_last_error());
    d_ids.Read(queue_, n * top, ids->data() + lo * top);
    d_terms.Read(queue_, n * top, terms->data() + lo * top);
    d_prob.Read(queue_, n, prob->data() + lo);
  }
  queue_.Finish();
}

void Learner::LinkCommunitySizes(Float min_term, std::vector<uint64_t>* sizes) {
  CheckLinkCommArgs("LinkCommunitySizes", 1, min_term);
  DrainAsync();
  queue_.Finish();
  const uint64_t K = pi_->Cols();
  sizes->assign(K + 1, 0);
  const std::vector<Edge> links = SortedTrainingLinks(cfg_);
  if (links.empty()) return;
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<Edge> d_edges(context, queue_, links.begin(), links.end());
  clcuda::Buffer<uint64_t> d_sizes(context, queue_, sizes->begin(), sizes->end());
  const int rc = ammsb_linkcomm_edges(&PostfitPi(), PostfitBeta(), MakeKernelParams(cfg_).epsilon, d_edges(), links.size(), 1,
                                      min_term, nullptr, nullptr, nullptr, d_sizes(), queue_.stream());
  if (rc != AMMSB_OK)
    throw PostfitError("ammsb_linkcomm_edges", rc, ammsb_linkcomm_last_error());
  d_sizes.Read(queue_, K + 1, sizes->data());
  queue_.Finish();
}

bool Learner::WriteLinkCommunities(std::ostream* out, uint32_t top, Float min_term) {
  const std::vector<Edge> links = SortedTrainingLinks(cfg_);
  std::vector<uint32_t> ids;
  std::vector<Float> terms, prob;
  LinkCommunities(links, top, min_term, &ids, &terms, &prob);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << links.size() << " " << top << " " << G9(min_term) << "\n";
  for (size_t i = 0; i < links.size(); ++i) {
    uint32_t n = 0;
    while (n < top && ids[i * top + n] != AMMSB_LINKCOMM_NONE) ++n;
    *out << (links[i] >> 32) << " " << (links[i] & 0xFFFFFFFFull) << " " << G9(prob[i]) << " " << n;
    for (uint32_t t = 0; t < n; ++t) *out << " " << ids[i * top + t] << " " << G9(terms[i * top + t]);
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- scoring communities against the graph: libammsb_quality.so over pi and the training links
void Learner::CommunityQuality(Float threshold, std::vector<uint64_t>* size, std::vector<uint64_t>* internal,
                               std::vector<uint64_t>* boundary, uint64_t* uncovered) {
  CheckThreshold("CommunityQuality", threshold);
  Memberships(1, threshold, nullptr, nullptr, nullptr, size);  // (drains; sizes only)
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  internal->assign(K, 0);
  boundary->assign(K, 0);
  *uncovered = 0;
  const std::vector<Edge> links = SortedTrainingLinks(cfg_);
  if (links.empty() || N == 0) return;
  const uint64_t words = ammsb_quality_mask_bytes(N, static_cast<uint32_t>(K)) / sizeof(uint64_t);
  if (words == 0) throw std::runtime_error("CommunityQuality: K outside 1..8192");
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<uint64_t> d_mask(context, words);
  clcuda::Buffer<Edge> d_edges(context, queue_, links.begin(), links.end());
  std::vector<uint64_t> counts(2 * K + 2, 0);
  clcuda::Buffer<uint64_t> d_counts(context, queue_, counts.begin(), counts.end());
  int rc = ammsb_quality_mask(&PostfitPi(), threshold, d_mask(), queue_.stream());
  if (rc == AMMSB_OK)
    rc = ammsb_quality_edges(d_mask(), N, static_cast<uint32_t>(K), d_edges(), links.size(), d_counts(), nullptr,
                             queue_.stream());
  if (rc != AMMSB_OK)
    throw PostfitError("ammsb_quality", rc, ammsb_quality_last_error());
  d_counts.Read(queue_, 2 * K + 2, counts.data());
  queue_.Finish();
  std::copy(counts.begin(), counts.begin() + K, internal->begin());
  std::copy(counts.begin() + K, counts.begin() + 2 * K, boundary->begin());
  *uncovered = counts[2 * K];
}

bool Learner::WriteCommunityQuality(std::ostream* out, Float threshold) {
  std::vector<uint64_t> size, internal, boundary;
  uint64_t uncovered = 0;
  CommunityQuality(threshold, &size, &internal, &boundary, &uncovered);
  const uint64_t links = SortedTrainingLinks(cfg_).size();  // (a training link has both ends < N: none is skipped)
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << links << " " << G9(threshold) << " " << uncovered << "\n";
  for (size_t k = 0; k < size.size(); ++k) {
    // float64, as include/ammsb_quality.h states the measures
    const uint64_t vol = 2 * internal[k] + boundary[k], low = std::min(vol, 2 * links - vol);
    const double cond = low ? static_cast<double>(boundary[k]) / static_cast<double>(low) : -1.0;
    const double sz = static_cast<double>(size[k]);
    const double dens = size[k] >= 2 ? static_cast<double>(internal[k]) / (sz * (sz - 1.0) / 2.0) : -1.0;
    *out << k << " " << size[k] << " " << internal[k] << " " << boundary[k] << " " << G9(cond) << " " << G9(dens) << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- matching the detected cover to a ground-truth cover: libammsb_cover.so over pi and the member list
void Learner::CoverMatch::Derive() {
  // one formula with _cover.py: F1 = 2 o / (t + d) in float64, the means added in index order
  const auto each = [](const std::vector<int32_t>& best, const std::vector<uint32_t>& over, auto own, auto other,
                       std::vector<double>* f1, double* mean) {
    f1->assign(best.size(), 0.0);
    double sum = 0;
    uint64_t present = 0;
    for (size_t i = 0; i < best.size(); ++i) {
      if (best[i] >= 0 && over[i] > 0)
        (*f1)[i] = 2.0 * static_cast<double>(over[i]) / (static_cast<double>(own(i)) + static_cast<double>(other(best[i])));
      if (own(i) > 0) {
        sum += (*f1)[i];
        ++present;
      }
    }
    *mean = present ? sum / static_cast<double>(present) : -1.0;
  };
  const auto t = [this](size_t g) { return static_cast<uint64_t>(truth_size[g]); };
  const auto d = [this](size_t k) { return detected_size[k]; };
  each(truth_best, truth_overlap, t, d, &f1_truth_each, &f1_truth);
  each(detected_best, detected_overlap, d, t, &f1_detected_each, &f1_detected);
  avg_f1 = f1_truth >= 0 && f1_detected >= 0 ? (f1_truth + f1_detected) / 2.0 : -1.0;
}

void Learner::CompareCover(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, Float threshold,
                           CoverMatch* m, std::vector<uint32_t>* overlap) {
  CheckThreshold("CompareCover", threshold);
  CheckTruthCover("CompareCover", offsets, members);
  const uint64_t G = offsets.size() - 1, M = members.size(), K = pi_->Cols();
  Memberships(1, threshold, nullptr, nullptr, nullptr, &m->detected_size);  // (drains; sizes only)
  m->truth_best.assign(G, -1);
  m->truth_overlap.assign(G, 0);
  m->truth_size.assign(G, 0);
  m->detected_best.assign(K, -1);
  m->detected_overlap.assign(K, 0);
  m->skipped = 0;
  if (overlap) overlap->assign(G * K, 0);
  if (G > 0 && M > 0) {  // (with nothing to compare the library launches nothing: every community is unmatched)
    const uint64_t ws_bytes = ammsb_cover_workspace_bytes(M, static_cast<uint32_t>(K));
    if (ws_bytes == 0) throw std::runtime_error("CompareCover: K outside 1..8192");
    const clcuda::Context context = queue_.GetContext();
    clcuda::Buffer<uint64_t> d_offsets(context, queue_, offsets.begin(), offsets.end());
    clcuda::Buffer<uint32_t> d_members(context, queue_, members.begin(), members.end());
    clcuda::Buffer<uint64_t> d_dsize(context, queue_, m->detected_size.begin(), m->detected_size.end());
    clcuda::Buffer<int32_t> d_tbest(context, G), d_dbest(context, K);
    clcuda::Buffer<uint32_t> d_tover(context, G), d_tsize(context, G), d_dover(context, K);
    clcuda::Buffer<uint32_t> d_dense(context, overlap ? G * K : 1);
    clcuda::Buffer<uint64_t> d_skipped(context, 1), d_ws(context, (ws_bytes + 7) / 8);
    const int rc = ammsb_cover_match(&PostfitPi(), threshold, d_offsets(), G, d_members(), M, d_dsize(), d_tbest(),
                                     d_tover(), d_tsize(), d_dbest(), d_dover(), d_skipped(),
                                     overlap ? d_dense() : nullptr, d_ws(), ws_bytes, queue_.stream());
    if (rc != AMMSB_OK)
      throw PostfitError("ammsb_cover_match", rc, ammsb_cover_last_error());
    d_tbest.Read(queue_, G, m->truth_best.data());
    d_tover.Read(queue_, G, m->truth_overlap.data());
    d_tsize.Read(queue_, G, m->truth_size.data());
    d_dbest.Read(queue_, K, m->detected_best.data());
    d_dover.Read(queue_, K, m->detected_overlap.data());
    d_skipped.Read(queue_, 1, &m->skipped);
    if (overlap) d_dense.Read(queue_, G * K, overlap->data());
    queue_.Finish();
  }
  m->Derive();
}

bool Learner::WriteCoverMatch(std::ostream* out, const std::vector<uint64_t>& offsets,
                              const std::vector<uint32_t>& members, Float threshold) {
  CoverMatch m;
  CompareCover(offsets, members, threshold, &m);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << m.truth_best.size() << " " << G9(threshold) << " "
       << m.skipped << " " << G9(m.f1_truth) << " " << G9(m.f1_detected) << " " << G9(m.avg_f1) << "\n";
  for (size_t g = 0; g < m.truth_best.size(); ++g)
    *out << "t " << g << " " << m.truth_size[g] << " " << m.truth_best[g] << " " << m.truth_overlap[g] << " "
         << G9(m.f1_truth_each[g]) << "\n";
  for (size_t k = 0; k < m.detected_best.size(); ++k)
    *out << "d " << k << " " << m.detected_size[k] << " " << m.detected_best[k] << " " << m.detected_overlap[k] << " "
         << G9(m.f1_detected_each[k]) << "\n";
  return static_cast<bool>(*out);
}

// ---- the overlapping NMI against a ground-truth cover: libammsb_cover.so for the dense overlap of a slab,
// libammsb_nmi.so for the pair pass
void Learner::CoverNmi::Derive() {
  // one formula with _nmi.py (include/ammsb_nmi.h), the sums added in index order
  const auto side = [](const std::vector<double>& H, const std::vector<double>& h, double* mean, double* sumH,
                       double* sumh) {
    double ratios = 0;
    uint64_t present = 0;
    *sumH = *sumh = 0;
    for (size_t i = 0; i < H.size(); ++i) {
      if (H[i] > 0) {
        ratios += h[i] / H[i];
        ++present;
      }
      *sumH += H[i];
      *sumh += h[i];
    }
    *mean = present ? ratios / static_cast<double>(present) : -1.0;
  };
  double mx, my, HX, hX, HY, hY;
  side(H_truth, h_truth, &mx, &HX, &hX);
  side(H_detected, h_detected, &my, &HY, &hY);
  nmi_lfk = mx < 0 || my < 0 ? -1.0 : 1.0 - 0.5 * (mx + my);
  const double den = std::max(HX, HY);
  nmi_max = den > 0 ? 0.5 * (HX - hX + HY - hY) / den : -1.0;
}

void Learner::CoverNMI(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, Float threshold,
                       CoverNmi* r, uint64_t slab_bytes) {
  CheckThreshold("CoverNMI", threshold);
  CheckTruthCover("CoverNMI", offsets, members);
  const uint64_t G = offsets.size() - 1, K = pi_->Cols(), N = pi_->Rows();
  CheckSets("CoverNMI", "NMI", offsets, members);
  Memberships(1, threshold, nullptr, nullptr, nullptr, &r->detected_size);  // (drains; sizes only)
  r->truth_size.assign(G, 0);
  r->skipped = 0;
  for (uint64_t g = 0; g < G; ++g)
    for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i) {
      if (members[i] < N) ++r->truth_size[g];
      else ++r->skipped;
    }
  r->H_truth.assign(G, 0);
  r->h_truth.assign(G, 0);
  r->H_detected.assign(K, 0);
  r->h_detected.assign(K, 0);
  if (K == 0 || K > AMMSB_NMI_MAX_COLS) throw std::runtime_error("CoverNMI: K outside 1..8192");
  const clcuda::Context context = queue_.GetContext();
  const uint64_t rows = std::min<uint64_t>(std::max<uint64_t>(G, 1), std::max<uint64_t>(1, slab_bytes / (4 * K)));
  uint64_t most_members = 1;  // of a slab
  for (uint64_t g0 = 0; g0 < G; g0 += rows)
    most_members = std::max(most_members, offsets[std::min(g0 + rows, G)] - offsets[g0]);
  const uint64_t ws_bytes = std::max<uint64_t>(8, ammsb_cover_workspace_bytes(most_members, static_cast<uint32_t>(K)));
  clcuda::Buffer<uint32_t> d_tsize(context, std::max<uint64_t>(G, 1));
  if (G) d_tsize.Write(queue_, G, r->truth_size.data());
  clcuda::Buffer<uint64_t> d_dsize(context, queue_, r->detected_size.begin(), r->detected_size.end());
  clcuda::Buffer<double> d_HX(context, std::max<uint64_t>(G, 1)), d_cX(context, std::max<uint64_t>(G, 1));
  clcuda::Buffer<double> d_HY(context, K), d_cY(context, K);
  int rc = ammsb_nmi_begin(N, d_tsize(), G, d_dsize(), static_cast<uint32_t>(K), d_HX(), d_HY(), d_cX(), d_cY(),
                           queue_.stream());
  if (rc != AMMSB_OK) throw PostfitError("ammsb_nmi_begin", rc, ammsb_nmi_last_error());
  if (G > 0) {
    clcuda::Buffer<uint64_t> d_offsets(context, rows + 1), d_skipped(context, 1), d_ws(context, (ws_bytes + 7) / 8);
    clcuda::Buffer<uint32_t> d_members(context, most_members), d_dense(context, rows * K);
    clcuda::Buffer<int32_t> d_tbest(context, rows), d_dbest(context, K);
    clcuda::Buffer<uint32_t> d_tover(context, rows), d_ts(context, rows), d_dover(context, K);
    std::vector<uint64_t> rebased;
    for (uint64_t g0 = 0; g0 < G; g0 += rows) {
      const uint64_t g1 = std::min(g0 + rows, G), Gs = g1 - g0, Ms = offsets[g1] - offsets[g0];
      if (Ms > 0) {
        rebased.assign(offsets.begin() + g0, offsets.begin() + g1 + 1);
        for (uint64_t& o : rebased) o -= offsets[g0];
        // (the host vectors are pageable: a write has returned when the device holds the data)
        d_offsets.Write(queue_, Gs + 1, rebased.data());
        d_members.Write(queue_, Ms, members.data() + offsets[g0]);
        rc = ammsb_cover_match(&PostfitPi(), threshold, d_offsets(), Gs, d_members(), Ms, d_dsize(), d_tbest(), d_tover(),
                               d_ts(), d_dbest(), d_dover(), d_skipped(), d_dense(), d_ws(), ws_bytes, queue_.stream());
        if (rc != AMMSB_OK) throw PostfitError("ammsb_cover_match", rc, ammsb_cover_last_error());
      } else {  // (the cover match launches nothing for communities without members: their overlap is 0)
        Zero("CoverNMI", d_dense(), Gs * K * sizeof(uint32_t), static_cast<hipStream_t>(queue_.stream()));
      }
      rc = ammsb_nmi_accumulate(d_dense(), g0, Gs, N, d_tsize(), G, d_dsize(), static_cast<uint32_t>(K), d_HX(), d_HY(),
                                d_cX(), d_cY(), queue_.stream());
      if (rc != AMMSB_OK) throw PostfitError("ammsb_nmi_accumulate", rc, ammsb_nmi_last_error());
    }
    d_HX.Read(queue_, G, r->H_truth.data());
    d_cX.Read(queue_, G, r->h_truth.data());
  }
  d_HY.Read(queue_, K, r->H_detected.data());
  d_cY.Read(queue_, K, r->h_detected.data());
  queue_.Finish();
  // the fallback: a community no pair qualifies for (+inf) keeps its own entropy
  for (uint64_t g = 0; g < G; ++g) r->h_truth[g] = std::min(r->h_truth[g], r->H_truth[g]);
  for (uint64_t k = 0; k < K; ++k) r->h_detected[k] = std::min(r->h_detected[k], r->H_detected[k]);
  r->Derive();
}

bool Learner::WriteCoverNMI(std::ostream* out, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members,
                            Float threshold, uint64_t slab_bytes) {
  CoverNmi r;
  CoverNMI(offsets, members, threshold, &r, slab_bytes);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.H_truth.size() << " " << G17(threshold) << " " << r.skipped
       << " " << G17(r.nmi_lfk) << " " << G17(r.nmi_max) << "\n";
  for (size_t g = 0; g < r.H_truth.size(); ++g)
    *out << "t " << g << " " << r.truth_size[g] << " " << G17(r.H_truth[g]) << " " << G17(r.h_truth[g]) << "\n";
  for (size_t k = 0; k < r.H_detected.size(); ++k)
    *out << "d " << k << " " << r.detected_size[k] << " " << G17(r.H_detected[k]) << " " << G17(r.h_detected[k]) << "\n";
  return static_cast<bool>(*out);
}

// ---- the Omega index against a ground-truth cover: libammsb_omega.so
namespace {
// num / den (den != 0, both below 2^127 in magnitude) rounded to binary64 once, to nearest even: 64 quotient bits by long division, the rest as a sticky
// bit.  What Python's int / int gives.
double RoundedQuotient(__int128 num, __int128 den) {
  typedef unsigned __int128 u128;
  if (num == 0) return 0.0;
  const bool neg = (num < 0) != (den < 0);
  const u128 a = num < 0 ? -static_cast<u128>(num) : static_cast<u128>(num);
  const u128 b = den < 0 ? -static_cast<u128>(den) : static_cast<u128>(den);
  u128 q = a / b, r = a % b;  // (r < b < 2^127: doubling it cannot wrap)
  int shift = 0;              // q holds floor(a 2^shift / b)
  bool sticky = false;
  while (q >> 64) {
    sticky = sticky || (q & 1);
    q >>= 1;
    --shift;
  }
  while (!(q >> 63)) {
    r <<= 1;
    q <<= 1;
    if (r >= b) {
      r -= b;
      q |= 1;
    }
    ++shift;
  }
  sticky = sticky || r != 0;
  uint64_t bits = static_cast<uint64_t>(q), keep = bits >> 11;
  const uint64_t low = bits & 0x7FF;
  if (low > 0x400 || (low == 0x400 && (sticky || (keep & 1)))) ++keep;
  const double v = std::ldexp(static_cast<double>(keep), 11 - shift);  // (keep <= 2^53: exact)
  return neg ? -v : v;
}
}  // namespace

void Learner::OmegaIndex::Derive() {
  // one formula with _omega.py (include/ammsb_omega.h): exact integers, the quotient rounded once
  const double nan = std::numeric_limits<double>::quiet_NaN();
  omega = omega_unadjusted = nan;
  if (nodes < 2) return;
  typedef __int128 i128;
  const i128 P = static_cast<i128>(nodes) * (nodes - 1) / 2;
  i128 Sa = 0, Se = 0;
  for (size_t j = 0; j < agree.size(); ++j) {
    Sa += agree[j];
    Se += static_cast<i128>(detected[j]) * truth[j];
  }
  omega_unadjusted = RoundedQuotient(Sa, P);
  const i128 den = P * P - Se;
  if (den != 0) omega = RoundedQuotient(Sa * P - Se, den);
}

std::vector<uint32_t> Learner::OmegaUniverse(const std::string& kind, const std::vector<uint32_t>& members, uint64_t N) {
  std::vector<uint32_t> u;
  if (kind == "all") {
    u.resize(N);
    for (uint64_t a = 0; a < N; ++a) u[a] = static_cast<uint32_t>(a);
  } else if (kind == "covered") {
    for (uint32_t m : members)
      if (m < N) u.push_back(m);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
  } else {
    throw std::invalid_argument("OmegaUniverse: the universe is \"covered\" or \"all\", not \"" + kind + "\"");
  }
  return u;
}

void Learner::CoverOmega(const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members, Float threshold,
                         const std::vector<uint32_t>& universe, OmegaIndex* r, uint64_t launch_pairs) {
  CheckThreshold("CoverOmega", threshold);
  CheckTruthCover("CoverOmega", offsets, members);
  const uint64_t G = offsets.size() - 1, M = members.size(), K = pi_->Cols(), N = pi_->Rows(), n = universe.size();
  if (launch_pairs < 1) throw std::invalid_argument("CoverOmega: launch_pairs must be at least 1");
  for (uint64_t i = 0; i < n; ++i)
    if (universe[i] >= N || (i > 0 && universe[i] <= universe[i - 1]))
      throw std::invalid_argument("CoverOmega: the universe ids must ascend, be distinct and < N");
  CheckSets("CoverOmega", "the Omega index", offsets, members);
  if (G > AMMSB_OMEGA_MAX_TRUTH) throw std::runtime_error("CoverOmega: more than 65536 ground-truth communities");
  if (K == 0 || K > AMMSB_OMEGA_MAX_COLS) throw std::runtime_error("CoverOmega: K outside 1..8192");
  DrainAsync();
  r->nodes = n;
  r->skipped = r->outside = 0;
  uint64_t L = 1;
  std::vector<uint64_t> hist(4, 0);
  if (n > 0) {
    const clcuda::Context context = queue_.GetContext();
    hipStream_t stream = static_cast<hipStream_t>(queue_.stream());
    const uint64_t WD = (K + 31) / 32, WT = (G + 31) / 32;
    std::vector<int32_t> position(N, -1);
    for (uint64_t i = 0; i < n; ++i) position[universe[i]] = static_cast<int32_t>(i);
    clcuda::Buffer<uint32_t> d_nodes(context, n), d_dbits(context, n * WD), d_tbits(context, std::max<uint64_t>(n * WT, 1));
    clcuda::Buffer<uint32_t> d_dcount(context, n), d_tcount(context, n), d_members(context, std::max<uint64_t>(M, 1));
    clcuda::Buffer<int32_t> d_position(context, N);
    clcuda::Buffer<uint64_t> d_offsets(context, G + 1), d_tally(context, 2);
    // (the host vectors are pageable: a write has returned when the device holds the data)
    d_nodes.Write(queue_, n, universe.data());
    d_position.Write(queue_, N, position.data());
    d_offsets.Write(queue_, G + 1, offsets.data());
    if (M) d_members.Write(queue_, M, members.data());
    Zero("CoverOmega", d_tbits(), std::max<uint64_t>(n * WT, 1) * sizeof(uint32_t), stream);
    Zero("CoverOmega", d_tcount(), n * sizeof(uint32_t), stream);
    Zero("CoverOmega", d_tally(), 2 * sizeof(uint64_t), stream);
    int rc = ammsb_omega_detected_bits(&PostfitPi(), threshold, d_nodes(), n, d_dbits(), d_dcount(), stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_omega_detected_bits", rc, ammsb_omega_last_error());
    rc = ammsb_omega_truth_bits(d_offsets(), G, d_members(), M, N, d_position(), n, d_tbits(), d_tcount(), d_tally(),
                                d_tally() + 1, stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_omega_truth_bits", rc, ammsb_omega_last_error());
    std::vector<uint32_t> dcount(n), tcount(n);
    std::vector<uint64_t> tally(2);
    d_dcount.Read(queue_, n, dcount.data());
    d_tcount.Read(queue_, n, tcount.data());
    d_tally.Read(queue_, 2, tally.data());
    queue_.Finish();
    r->skipped = tally[0];
    r->outside = tally[1];
    L = 1 + std::max<uint64_t>(*std::max_element(dcount.begin(), dcount.end()),
                               *std::max_element(tcount.begin(), tcount.end()));
    if (L > AMMSB_OMEGA_MAX_LEVELS) throw std::runtime_error("CoverOmega: a node of the universe is in more than 4095 communities");
    hist.assign(3 * L + 1, 0);
    clcuda::Buffer<uint64_t> d_hist(context, 3 * L + 1);
    Zero("CoverOmega", d_hist(), (3 * L + 1) * sizeof(uint64_t), stream);
    const uint64_t R = (n + AMMSB_OMEGA_TILE - 1) / AMMSB_OMEGA_TILE, total = R * (R + 1) / 2;
    const uint64_t step = std::min<uint64_t>(
        AMMSB_OMEGA_MAX_LAUNCH_TILES, std::max<uint64_t>(1, launch_pairs / (uint64_t(AMMSB_OMEGA_TILE) * AMMSB_OMEGA_TILE)));
    for (uint64_t t0 = 0; t0 < total; t0 += step) {
      rc = ammsb_omega_pairs(d_dbits(), static_cast<uint32_t>(K), d_tbits(), G, n, static_cast<uint32_t>(L), t0,
                             std::min(step, total - t0), d_hist(), stream);
      if (rc != AMMSB_OK) throw PostfitError("ammsb_omega_pairs", rc, ammsb_omega_last_error());
    }
    d_hist.Read(queue_, 3 * L + 1, hist.data());
    queue_.Finish();
    if (hist[3 * L] != 0) throw std::runtime_error("CoverOmega: pairs past the highest level any node reaches");
  } else {
    for (uint32_t m : members) r->skipped += m >= N, r->outside += m < N;
  }
  r->agree.assign(hist.begin(), hist.begin() + L);
  r->detected.assign(hist.begin() + L, hist.begin() + 2 * L);
  r->truth.assign(hist.begin() + 2 * L, hist.begin() + 3 * L);
  r->Derive();
}

bool Learner::WriteCoverOmega(std::ostream* out, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& members,
                              Float threshold, const std::vector<uint32_t>& universe, uint64_t launch_pairs) {
  OmegaIndex r;
  CoverOmega(offsets, members, threshold, universe, &r, launch_pairs);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << offsets.size() - 1 << " " << G17(threshold) << " " << r.nodes
       << " " << r.skipped << " " << r.outside << " " << G17(r.omega) << " " << G17(r.omega_unadjusted) << "\n";
  for (size_t j = 0; j < r.agree.size(); ++j)
    *out << j << " " << r.agree[j] << " " << r.detected[j] << " " << r.truth[j] << "\n";
  return static_cast<bool>(*out);
}


// ---- how the detected communities relate to each other: libammsb_relate.so over slabs of pi
namespace {
uint32_t RelateMeasure(const std::string& by) {
  if (by == "overlap") return AMMSB_RELATE_OVERLAP;
  if (by == "jaccard") return AMMSB_RELATE_JACCARD;
  if (by == "contained") return AMMSB_RELATE_CONTAINED;
  throw std::invalid_argument("RelatedCommunities: the measure is \"overlap\", \"jaccard\" or \"contained\", not \"" + by + "\"");
}

// overlap[K, K] on the device, slab by slab; the stream is left running
void OverlapOnDevice(const ammsb_rpm* pi, Float threshold, uint64_t max_bytes, clcuda::Buffer<uint32_t>* d_overlap,
                     const clcuda::Context& context, void* stream) {
  const uint64_t N = pi->num_rows, K = pi->num_cols;
  if (K == 0 || K > AMMSB_RELATE_MAX_COLS) throw std::runtime_error("CommunityOverlap: K outside 1..8192");
  Zero("CommunityOverlap", (*d_overlap)(), K * K * sizeof(uint32_t), static_cast<hipStream_t>(stream));
  if (N == 0) return;
  const uint64_t step = std::min<uint64_t>((N + 63) / 64 * 64, std::max<uint64_t>(64, max_bytes * 8 / K / 64 * 64));
  clcuda::Buffer<uint64_t> d_bits(context, K * (step / 64));
  for (uint64_t lo = 0; lo < N; lo += step) {
    const uint64_t n = std::min(step, N - lo);
    int rc = ammsb_relate_bits(pi, threshold, lo, n, d_bits(), stream);
    if (rc == AMMSB_OK) rc = ammsb_relate_pairs(d_bits(), static_cast<uint32_t>(K), n, (*d_overlap)(), stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_relate", rc, ammsb_relate_last_error());
  }
  // d_bits is freed on return: the slabs have to be through with it
  const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if (e != hipSuccess) throw std::runtime_error(std::string("CommunityOverlap: ") + hipGetErrorString(e));
}
}  // namespace

void Learner::CommunityOverlap(Float threshold, std::vector<uint32_t>* overlap, uint64_t max_bytes) {
  CheckThreshold("CommunityOverlap", threshold);
  if (max_bytes < 1) throw std::invalid_argument("CommunityOverlap: max_bytes must be at least 1");
  DrainAsync();
  queue_.Finish();
  const uint64_t K = pi_->Cols();
  clcuda::Buffer<uint32_t> d_overlap(queue_.GetContext(), K * K);
  OverlapOnDevice(&PostfitPi(), threshold, max_bytes, &d_overlap, queue_.GetContext(), queue_.stream());
  overlap->resize(K * K);
  d_overlap.Read(queue_, K * K, overlap->data());
  queue_.Finish();
}

void Learner::RelatedCommunities(Float threshold, uint32_t top, const std::string& by, uint32_t min_overlap,
                                 Related* related, uint64_t max_bytes) {
  CheckThreshold("RelatedCommunities", threshold);
  const uint32_t measure = RelateMeasure(by);
  if (top == 0 || top > AMMSB_RELATE_MAX_TOP) throw std::invalid_argument("RelatedCommunities: top must be in 1..64");
  if (max_bytes < 1) throw std::invalid_argument("RelatedCommunities: max_bytes must be at least 1");
  DrainAsync();
  queue_.Finish();
  const uint64_t K = pi_->Cols();
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<uint32_t> d_overlap(context, K * K), d_shared(context, K * top);
  clcuda::Buffer<int32_t> d_partner(context, K * top);
  OverlapOnDevice(&PostfitPi(), threshold, max_bytes, &d_overlap, context, queue_.stream());
  const int rc = ammsb_relate_top(d_overlap(), static_cast<uint32_t>(K), measure, top, min_overlap, d_partner(), d_shared(),
                                  queue_.stream());
  if (rc != AMMSB_OK) throw PostfitError("ammsb_relate_top", rc, ammsb_relate_last_error());
  related->partner.resize(K * top);
  related->overlap.resize(K * top);
  d_partner.Read(queue_, K * top, related->partner.data());
  d_shared.Read(queue_, K * top, related->overlap.data());
  std::vector<uint32_t> matrix(K * K);
  d_overlap.Read(queue_, K * K, matrix.data());
  queue_.Finish();
  related->size.resize(K);
  for (uint64_t k = 0; k < K; ++k) related->size[k] = matrix[k * K + k];
}

bool Learner::WriteRelatedCommunities(std::ostream* out, Float threshold, uint32_t top, const std::string& by,
                                      uint32_t min_overlap, uint64_t max_bytes) {
  Related r;
  RelatedCommunities(threshold, top, by, min_overlap, &r, max_bytes);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << G9(threshold) << " " << by << " " << top << " " << min_overlap
       << "\n";
  for (size_t k = 0; k < r.size.size(); ++k) {
    uint32_t n = 0;
    while (n < top && r.partner[k * top + n] >= 0) ++n;
    *out << k << " " << r.size[k] << " " << n;
    for (uint32_t t = 0; t < n; ++t) *out << " " << r.partner[k * top + t] << " " << r.overlap[k * top + t];
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- how the detected communities are linked to each other: libammsb_connect.so over pi and the training links
namespace {
uint32_t ConnectMeasure(const std::string& by) {
  if (by == "links") return AMMSB_CONNECT_LINKS;
  if (by == "density") return AMMSB_CONNECT_DENSITY;
  throw std::invalid_argument("LinkedCommunities: the measure is \"links\" or \"density\", not \"" + by + "\"");
}

// links[K, K] and counts[2] on the device from the sorted training links; waits before it returns (the mask, the edge
// list and the directed matrix are freed on return)
void LinksOnDevice(const ammsb_rpm* pi, Float threshold, const std::vector<Edge>& edges, clcuda::Buffer<uint64_t>* d_links,
                   clcuda::Buffer<uint64_t>* d_counts, const clcuda::Context& context, const clcuda::Queue& queue) {
  const uint64_t N = pi->num_rows, K = pi->num_cols;
  if (K == 0 || K > AMMSB_CONNECT_MAX_COLS) throw std::runtime_error("CommunityLinks: K outside 1..8192");
  hipStream_t stream = static_cast<hipStream_t>(queue.stream());
  clcuda::Buffer<uint64_t> d_directed(context, K * K);
  Zero("CommunityLinks", d_directed(), K * K * sizeof(uint64_t), stream);
  Zero("CommunityLinks", (*d_counts)(), 2 * sizeof(uint64_t), stream);
  // without an edge or a node the mask is not made and no edge kernel runs (the keys are uploaded before the mask pass)
  const bool any = !edges.empty() && N > 0;
  std::unique_ptr<clcuda::Buffer<Edge>> d_edges;
  if (any) d_edges.reset(new clcuda::Buffer<Edge>(context, queue, edges.begin(), edges.end()));
  const clcuda::Buffer<uint64_t> d_mask = MembershipMask("ammsb_connect", pi, threshold, context, stream, any);
  int rc = AMMSB_OK;
  if (any)
    rc = ammsb_connect_edges(d_mask(), N, static_cast<uint32_t>(K), (*d_edges)(), edges.size(), d_directed(), (*d_counts)(),
                             stream);
  if (rc == AMMSB_OK) rc = ammsb_connect_finish(d_directed(), static_cast<uint32_t>(K), (*d_links)(), stream);
  if (rc != AMMSB_OK) throw PostfitError("ammsb_connect", rc, ammsb_connect_last_error());
  const hipError_t e = hipStreamSynchronize(stream);
  if (e != hipSuccess) throw std::runtime_error(std::string("CommunityLinks: ") + hipGetErrorString(e));
}
}  // namespace

void Learner::CommunityLinks(Float threshold, std::vector<uint64_t>* links) {
  CheckThreshold("CommunityLinks", threshold);
  DrainAsync();
  queue_.Finish();
  const uint64_t K = pi_->Cols();
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<uint64_t> d_links(context, K * K), d_counts(context, 2);
  LinksOnDevice(&PostfitPi(), threshold, SortedTrainingLinks(cfg_), &d_links, &d_counts, context, queue_);
  links->resize(K * K);
  d_links.Read(queue_, K * K, links->data());
  queue_.Finish();
}

void Learner::LinkedCommunities(Float threshold, uint32_t top, const std::string& by, uint64_t min_links, Linked* linked,
                                uint64_t max_bytes) {
  CheckThreshold("LinkedCommunities", threshold);
  const uint32_t measure = ConnectMeasure(by);
  if (top == 0 || top > AMMSB_CONNECT_MAX_TOP) throw std::invalid_argument("LinkedCommunities: top must be in 1..64");
  if (max_bytes < 1) throw std::invalid_argument("LinkedCommunities: max_bytes must be at least 1");
  DrainAsync();
  queue_.Finish();
  const uint64_t K = pi_->Cols();
  const clcuda::Context context = queue_.GetContext();
  clcuda::Buffer<uint32_t> d_overlap(context, K * K), d_shared(context, K * top);
  clcuda::Buffer<uint64_t> d_links(context, K * K), d_counts(context, 2), d_plinks(context, K * top);
  clcuda::Buffer<int32_t> d_partner(context, K * top);
  OverlapOnDevice(&PostfitPi(), threshold, max_bytes, &d_overlap, context, queue_.stream());
  LinksOnDevice(&PostfitPi(), threshold, SortedTrainingLinks(cfg_), &d_links, &d_counts, context, queue_);
  const int rc = ammsb_connect_top(d_links(), d_overlap(), static_cast<uint32_t>(K), measure, top, min_links, d_partner(),
                                   d_plinks(), d_shared(), queue_.stream());
  if (rc != AMMSB_OK) throw PostfitError("ammsb_connect_top", rc, ammsb_connect_last_error());
  linked->partner.resize(K * top);
  linked->links.resize(K * top);
  linked->shared.resize(K * top);
  d_partner.Read(queue_, K * top, linked->partner.data());
  d_plinks.Read(queue_, K * top, linked->links.data());
  d_shared.Read(queue_, K * top, linked->shared.data());
  std::vector<uint32_t> overlap(K * K);
  std::vector<uint64_t> matrix(K * K), counts(2);
  d_overlap.Read(queue_, K * K, overlap.data());
  d_links.Read(queue_, K * K, matrix.data());
  d_counts.Read(queue_, 2, counts.data());
  queue_.Finish();
  linked->size.resize(K);
  linked->internal.resize(K);
  for (uint64_t k = 0; k < K; ++k) {
    linked->size[k] = overlap[k * K + k];
    linked->internal[k] = matrix[k * K + k] / 2;
  }
  linked->valid = counts[0];
  linked->skipped = counts[1];
}

bool Learner::WriteLinkedCommunities(std::ostream* out, Float threshold, uint32_t top, const std::string& by,
                                     uint64_t min_links, uint64_t max_bytes) {
  Linked r;
  LinkedCommunities(threshold, top, by, min_links, &r, max_bytes);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.valid + r.skipped << " " << G9(threshold) << " " << by << " "
       << top << " " << min_links << " " << r.skipped << "\n";
  for (size_t k = 0; k < r.size.size(); ++k) {
    uint32_t n = 0;
    while (n < top && r.partner[k * top + n] >= 0) ++n;
    *out << k << " " << r.size[k] << " " << r.internal[k] << " " << n;
    for (uint32_t t = 0; t < n; ++t)
      *out << " " << r.partner[k * top + t] << " " << r.links[k * top + t] << " " << r.shared[k * top + t];
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- is the cover better than chance: libammsb_modularity.so over libammsb_connect.so's mask of pi and an edge list
void Learner::ModularityScore::Derive() {
#pragma STDC FP_CONTRACT OFF
  const size_t K = internal.size();
  in_each.resize(K);
  s_each.resize(K);
  q_each.assign(K, -1.0);
  q = -1.0;
  for (size_t k = 0; k < K; ++k) {
    // (the conversion of a 128-bit integer rounds once, to nearest even; the scaling is exact)
    in_each[k] = std::ldexp(static_cast<double>(internal[k]), -static_cast<int>(AMMSB_MODULARITY_FRAC_BITS));
    s_each[k] = std::ldexp(static_cast<double>(volume[k]), -static_cast<int>(AMMSB_MODULARITY_FRAC_BITS));
  }
  if (links == 0) return;
  const double two_m = static_cast<double>(2 * links);
  q = 0.0;
  for (size_t k = 0; k < K; ++k) {
    const double twice = 2.0 * in_each[k];
    const double square = s_each[k] * s_each[k];
    const double chance = square / two_m;
    const double diff = twice - chance;
    q_each[k] = diff / two_m;
    q += q_each[k];
  }
}

void Learner::Modularity(Float threshold, const std::vector<Edge>* edges, ModularityScore* result) {
  CheckThreshold("Modularity", threshold);
  if (edges && edges->size() >= AMMSB_MODULARITY_MAX_EDGES)
    throw std::invalid_argument("Modularity: an edge list of 2^31 keys or more");
  DrainAsync();
  queue_.Finish();
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  if (K == 0 || K > AMMSB_MODULARITY_MAX_COLS) throw std::runtime_error("Modularity: K outside 1..8192");
  std::vector<Edge> training;
  edges = EdgesOrTraining("Modularity", edges, cfg_, &training, AMMSB_MODULARITY_MAX_EDGES);
  result->internal.assign(K, 0);
  result->volume.assign(K, 0);
  result->degree.assign(N, 0);
  result->links = 0;
  result->skipped = edges->size();  // (without a node every key has an end >= N)
  if (!edges->empty() && N > 0) {
    hipStream_t stream = static_cast<hipStream_t>(queue_.stream());
    const clcuda::Context context = queue_.GetContext();
    clcuda::Buffer<uint64_t> d_sums(context, 4 * K + 2);  // internal, volume, counts
    clcuda::Buffer<uint32_t> d_degree(context, N);
    clcuda::Buffer<Edge> d_edges(context, queue_, edges->begin(), edges->end());
    Zero("Modularity", d_sums(), (4 * K + 2) * sizeof(uint64_t), stream);
    Zero("Modularity", d_degree(), N * sizeof(uint32_t), stream);
    const clcuda::Buffer<uint64_t> d_mask = MembershipMask("ammsb_connect_mask", &PostfitPi(), threshold, context, stream);
    int rc = ammsb_modularity_edges(d_mask(), N, static_cast<uint32_t>(K), d_edges(), edges->size(), d_degree(), d_sums(),
                                d_sums() + 4 * K, stream);
    if (rc == AMMSB_OK)
      rc = ammsb_modularity_nodes(d_mask(), N, static_cast<uint32_t>(K), d_degree(), d_sums() + 2 * K, stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_modularity", rc, ammsb_modularity_last_error());
    std::vector<uint64_t> sums(4 * K + 2);
    d_sums.Read(queue_, 4 * K + 2, sums.data());
    d_degree.Read(queue_, N, result->degree.data());
    queue_.Finish();
    typedef unsigned __int128 u128;
    for (uint64_t k = 0; k < K; ++k) {
      result->internal[k] = (static_cast<u128>(sums[2 * k + 1]) << 64) | sums[2 * k];
      result->volume[k] = (static_cast<u128>(sums[2 * K + 2 * k + 1]) << 64) | sums[2 * K + 2 * k];
    }
    result->links = sums[4 * K];
    result->skipped = sums[4 * K + 1];
  }
  result->Derive();
}

bool Learner::WriteModularity(std::ostream* out, Float threshold, const std::vector<Edge>* edges) {
  ModularityScore r;
  Modularity(threshold, edges, &r);
  const auto hex = [](unsigned __int128 v) {
    char buf[40];
    snprintf(buf, sizeof(buf), "%016llx%016llx", static_cast<unsigned long long>(v >> 64), static_cast<unsigned long long>(v));
    return std::string(buf);
  };
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.links + r.skipped << " " << G9(threshold) << " " << r.skipped
       << " " << G17(r.q) << "\n";
  for (size_t k = 0; k < r.q_each.size(); ++k)
    *out << k << " " << G17(r.q_each[k]) << " " << G17(r.in_each[k]) << " " << G17(r.s_each[k]) << " " << hex(r.internal[k])
         << " " << hex(r.volume[k]) << "\n";
  return static_cast<bool>(*out);
}

// ---- how does a single node sit in the cover: libammsb_roles.so over libammsb_connect.so's mask of pi and a CSR adjacency
void Learner::NodeRolesResult::Derive() {
#pragma STDC FP_CONTRACT OFF
  const size_t n = degree.size(), K = ksum.size();
  embeddedness.assign(n, -1.0);
  participation.assign(n, -1.0);
  z.assign(n * top, 0.0);
  // (every integer is converted once, to nearest even)
  std::vector<double> mean(K, 0.0), sigma(K, 0.0);  // sigma 0: no z in this community
  for (size_t k = 0; k < K; ++k) {
    if (kmembers[k] < 2) continue;
    const double members = static_cast<double>(kmembers[k]);
    mean[k] = static_cast<double>(ksum[k]) / members;
    const double second = static_cast<double>(ksq[k]) / members;
    const double square = mean[k] * mean[k];
    const double var = second - square;
    if (var > 0) sigma[k] = std::sqrt(var);
  }
  for (size_t i = 0; i < n; ++i) {
    if (degree[i] > 0) embeddedness[i] = static_cast<double>(embedded[i]) / static_cast<double>(degree[i]);
    if (votes[i] > 0) {
      const double v = static_cast<double>(votes[i]);
      const double vv = v * v;
      const double ratio = static_cast<double>(squares[i]) / vv;
      participation[i] = 1.0 - ratio;
    }
    for (uint32_t j = 0; j < top; ++j) {
      const int32_t k = home[i * top + j];
      if (k < 0 || !(sigma[k] > 0)) continue;
      const double diff = static_cast<double>(hcount[i * top + j]) - mean[k];
      z[i * top + j] = diff / sigma[k];
    }
  }
}

void Learner::NodeRoles(Float threshold, const std::vector<Edge>* edges, uint32_t top, const std::string& among,
                        uint32_t min_count, NodeRolesResult* result) {
  CheckThreshold("NodeRoles", threshold);
  if (top == 0 || top > AMMSB_ROLES_MAX_TOP) throw std::invalid_argument("NodeRoles: top must be in 1..16");
  if (among != "all" && among != "own") throw std::invalid_argument("NodeRoles: among must be \"all\" or \"own\"");
  DrainAsync();
  queue_.Finish();
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  if (K == 0 || K > AMMSB_ROLES_MAX_COLS) throw std::runtime_error("NodeRoles: K outside 1..8192");
  // the adjacency: the training graph's rows, or both directions of every valid key of the list, in the list's order
  std::vector<uint64_t> offsets;
  std::vector<Vertex> targets;
  uint64_t lost = 0;  // keys with an end >= N
  if (!edges) {
    cfg_.trainingGraph->ExportCSR(&offsets, &targets);
  } else {
    offsets.assign(N + 1, 0);
    for (Edge e : *edges) {
      const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
      if (a >= N || b >= N) {
        ++lost;
        continue;
      }
      ++offsets[a + 1];
      ++offsets[b + 1];
    }
    for (uint64_t a = 0; a < N; ++a) offsets[a + 1] += offsets[a];
    targets.resize(offsets[N]);
    std::vector<uint64_t> at(offsets.begin(), offsets.end() - 1);
    for (Edge e : *edges) {
      const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
      if (a >= N || b >= N) continue;
      targets[at[a]++] = static_cast<Vertex>(b);
      targets[at[b]++] = static_cast<Vertex>(a);
    }
  }
  if (offsets.size() != N + 1) throw std::runtime_error("NodeRoles: the adjacency does not have N rows");
  for (uint64_t a = 0; a < N; ++a)
    if (offsets[a + 1] - offsets[a] > AMMSB_ROLES_MAX_ROW) throw std::invalid_argument("NodeRoles: a row of more than 2^25 targets");
  NodeRolesResult& r = *result;
  r.top = top;
  r.degree.assign(N, 0);
  r.own.assign(N, 0);
  r.embedded.assign(N, 0);
  r.reached.assign(N, 0);
  r.votes.assign(N, 0);
  r.squares.assign(N, 0);
  r.home.assign(N * top, -1);
  r.hcount.assign(N * top, 0);
  r.hflags.assign(N, 0);
  r.ksum.assign(K, 0);
  r.ksq.assign(K, 0);
  r.kmembers.assign(K, 0);
  r.valid = 0;
  r.skipped = lost;
  if (N > 0) {
    hipStream_t stream = static_cast<hipStream_t>(queue_.stream());
    const clcuda::Context context = queue_.GetContext();
    if (targets.empty()) targets.push_back(0);  // (a buffer needs a byte; no offset reaches it)
    clcuda::Buffer<uint64_t> d_sums(context, 3 * K + 2), d_wide(context, 2 * N);  // ksum ksq kmembers counts; votes squares
    clcuda::Buffer<uint32_t> d_node(context, 5 * N), d_slots(context, 2 * N * top);  // degree own embedded reached hflags; home hcount
    clcuda::Buffer<uint64_t> d_offsets(context, queue_, offsets.begin(), offsets.end());
    clcuda::Buffer<Vertex> d_targets(context, queue_, targets.begin(), targets.end());
    Zero("NodeRoles", d_sums(), (3 * K + 2) * sizeof(uint64_t), stream);
    const clcuda::Buffer<uint64_t> d_mask = MembershipMask("ammsb_connect_mask", &PostfitPi(), threshold, context, stream);
    int rc = ammsb_roles_nodes(d_mask(), N, static_cast<uint32_t>(K), d_offsets(), d_targets(), 0, N,
                           among == "own" ? AMMSB_ROLES_OWN : AMMSB_ROLES_ALL, top, min_count, d_node(), d_node() + N,
                           d_node() + 2 * N, d_node() + 3 * N, d_wide(), d_wide() + N, reinterpret_cast<int32_t*>(d_slots()),
                           d_slots() + N * top, d_node() + 4 * N, d_sums(), d_sums() + K, d_sums() + 2 * K, d_sums() + 3 * K,
                           stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_roles_nodes", rc, ammsb_roles_last_error());
    std::vector<uint64_t> sums(3 * K + 2), wide(2 * N);
    std::vector<uint32_t> node(5 * N), slots(2 * N * top);
    d_sums.Read(queue_, 3 * K + 2, sums.data());
    d_wide.Read(queue_, 2 * N, wide.data());
    d_node.Read(queue_, 5 * N, node.data());
    d_slots.Read(queue_, 2 * N * top, slots.data());
    queue_.Finish();
    r.degree.assign(node.begin(), node.begin() + N);
    r.own.assign(node.begin() + N, node.begin() + 2 * N);
    r.embedded.assign(node.begin() + 2 * N, node.begin() + 3 * N);
    r.reached.assign(node.begin() + 3 * N, node.begin() + 4 * N);
    r.hflags.assign(node.begin() + 4 * N, node.end());
    r.votes.assign(wide.begin(), wide.begin() + N);
    r.squares.assign(wide.begin() + N, wide.end());
    for (uint64_t i = 0; i < N * top; ++i) r.home[i] = static_cast<int32_t>(slots[i]);
    r.hcount.assign(slots.begin() + N * top, slots.end());
    r.ksum.assign(sums.begin(), sums.begin() + K);
    r.ksq.assign(sums.begin() + K, sums.begin() + 2 * K);
    r.kmembers.assign(sums.begin() + 2 * K, sums.begin() + 3 * K);
    r.valid = sums[3 * K];
    r.skipped = lost + sums[3 * K + 1];
  }
  r.Derive();
}

bool Learner::WriteNodeRoles(std::ostream* out, Float threshold, uint32_t top, const std::string& among, uint32_t min_count,
                             const std::vector<Edge>* edges) {
  NodeRolesResult r;
  NodeRoles(threshold, edges, top, among, min_count, &r);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.valid + r.skipped << " " << G9(threshold) << " " << among << " "
       << top << " " << min_count << " " << r.skipped << "\n";
  for (size_t k = 0; k < r.ksum.size(); ++k)
    *out << "c " << k << " " << r.kmembers[k] << " " << r.ksum[k] << " " << r.ksq[k] << "\n";
  for (size_t a = 0; a < r.degree.size(); ++a) {
    uint32_t filled = 0;
    while (filled < top && r.home[a * top + filled] >= 0) ++filled;
    *out << "n " << a << " " << r.degree[a] << " " << r.own[a] << " " << r.embedded[a] << " " << r.reached[a] << " " << r.votes[a]
         << " " << r.squares[a] << " " << filled;
    for (uint32_t j = 0; j < filled; ++j)
      *out << " " << r.home[a * top + j] << " " << r.hcount[a * top + j] << " " << ((r.hflags[a] >> j) & 1u);
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- do the communities hold triangles: libammsb_triangles.so and libammsb_roles.so over libammsb_connect.so's mask of pi
// and one simple CSR adjacency
void Learner::TrianglesResult::Derive() {
#pragma STDC FP_CONTRACT OFF
  const size_t n = degree.size(), K = ktri3.size();
  // (every integer is converted once, to nearest even)
  uint64_t sum_tri = 0, all_pairs = 0;
  for (size_t i = 0; i < n; ++i) sum_tri += tri[i];
  if (sum_tri % 3) throw std::logic_error("Triangles: the nodes' triangles are not a multiple of 3");
  tpr.assign(K, -1.0);
  clustering.assign(K, -1.0);
  triangles.assign(K, 0);
  for (size_t k = 0; k < K; ++k) {
    if (ktri3[k] % 3) throw std::logic_error("Triangles: ktri3 is not a multiple of 3");
    triangles[k] = ktri3[k] / 3;
    if (kmembers[k] > 0) tpr[k] = static_cast<double>(kpart[k]) / static_cast<double>(kmembers[k]);
    if (wedges[k] > 0) clustering[k] = static_cast<double>(ktri3[k]) / static_cast<double>(wedges[k]);
  }
  local_clustering.assign(n, -1.0);
  inside.assign(n, -1.0);
  double sum_local = 0;
  uint64_t some = 0;
  for (size_t i = 0; i < n; ++i) {
    if (degree[i] >= 2) {
      const double d = static_cast<double>(degree[i]);
      const double less = d - 1.0;
      const double product = d * less;
      const double pairs = product / 2.0;
      local_clustering[i] = static_cast<double>(tri[i]) / pairs;
      sum_local += local_clustering[i];
      ++some;
      all_pairs += static_cast<uint64_t>(degree[i]) * (degree[i] - 1) / 2;
    }
    if (tri[i] > 0) inside[i] = static_cast<double>(tri_in[i]) / static_cast<double>(tri[i]);
  }
  total = sum_tri / 3;
  transitivity = all_pairs ? static_cast<double>(sum_tri) / static_cast<double>(all_pairs) : -1.0;
  avg_clustering = some ? sum_local / static_cast<double>(some) : -1.0;
}

// The simple adjacency of a key list, which Triangles and CommunityCores share: both directions of every key with both ends
// < N, each row sorted and made unique, loops left out.  *valid: the keys with both ends < N; *lost: those with an end >= N.
// max_row > 0: std::invalid_argument(too_long) on a longer row.
static void SimpleAdjacency(const std::vector<Edge>& list, uint64_t N, uint64_t max_row, const char* too_long,
                            std::vector<uint64_t>* offsets, std::vector<Vertex>* targets, uint64_t* valid, uint64_t* lost) {
  std::vector<std::vector<Vertex>> rows(N);
  *valid = *lost = 0;
  for (Edge e : list) {
    const uint64_t a = e >> 32, b = e & 0xFFFFFFFFull;
    if (a >= N || b >= N) {
      ++*lost;
      continue;
    }
    ++*valid;
    if (a == b) continue;
    rows[a].push_back(static_cast<Vertex>(b));
    rows[b].push_back(static_cast<Vertex>(a));
  }
  offsets->assign(N + 1, 0);
  targets->clear();
  for (uint64_t a = 0; a < N; ++a) {
    std::sort(rows[a].begin(), rows[a].end());
    rows[a].erase(std::unique(rows[a].begin(), rows[a].end()), rows[a].end());
    if (max_row && rows[a].size() > max_row) throw std::invalid_argument(too_long);
    targets->insert(targets->end(), rows[a].begin(), rows[a].end());
    (*offsets)[a + 1] = targets->size();
    std::vector<Vertex>().swap(rows[a]);
  }
}

void Learner::Triangles(Float threshold, const std::vector<Edge>* edges, TrianglesResult* result) {
  CheckThreshold("Triangles", threshold);
  DrainAsync();
  queue_.Finish();
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  if (K == 0 || K > AMMSB_TRIANGLES_MAX_COLS) throw std::runtime_error("Triangles: K outside 1..8192");
  // the simple adjacency: both directions of every valid key, each row sorted and made unique, loops left out
  std::vector<Edge> training;
  const std::vector<Edge>& list = *EdgesOrTraining("Triangles", edges, cfg_, &training);
  std::vector<uint64_t> offsets;
  std::vector<Vertex> targets;
  uint64_t valid = 0, lost = 0;  // keys with both ends < N; with an end >= N
  SimpleAdjacency(list, N, AMMSB_TRIANGLES_MAX_ROW, "Triangles: a row of more than 65535 targets", &offsets, &targets, &valid, &lost);
  TrianglesResult& r = *result;
  r.M = targets.size();
  r.skipped = lost;
  r.dropped = valid - r.M / 2;
  r.degree.assign(N, 0);
  r.tri.assign(N, 0);
  r.tri_in.assign(N, 0);
  r.tri_comms.assign(N, 0);
  r.ktri3.assign(K, 0);
  r.kpart.assign(K, 0);
  r.kmembers.assign(K, 0);
  r.wedges.assign(K, 0);
  if (N > 0) {
    hipStream_t stream = static_cast<hipStream_t>(queue_.stream());
    const clcuda::Context context = queue_.GetContext();
    if (targets.empty()) targets.push_back(0);  // (a buffer needs a byte; no offset reaches it)
    // ktri3 kpart counts, then the node roles' ksum ksq kmembers counts; votes squares
    clcuda::Buffer<uint64_t> d_sums(context, 5 * K + 4), d_wide(context, 2 * N);
    clcuda::Buffer<uint32_t> d_node(context, 7 * N);  // tri tri_in tri_comms; degree own embedded reached
    clcuda::Buffer<uint64_t> d_offsets(context, queue_, offsets.begin(), offsets.end());
    clcuda::Buffer<Vertex> d_targets(context, queue_, targets.begin(), targets.end());
    Zero("Triangles", d_sums(), (5 * K + 4) * sizeof(uint64_t), stream);
    const clcuda::Buffer<uint64_t> d_mask = MembershipMask("ammsb_connect_mask", &PostfitPi(), threshold, context, stream);
    int rc = ammsb_triangles_nodes(d_mask(), N, static_cast<uint32_t>(K), d_offsets(), d_targets(), 0, N, d_node(), d_node() + N,
                               d_node() + 2 * N, d_sums(), d_sums() + K, d_sums() + 2 * K, stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_triangles_nodes", rc, ammsb_triangles_last_error());
    uint64_t* const roles = d_sums() + 2 * K + 2;
    rc = ammsb_roles_nodes(d_mask(), N, static_cast<uint32_t>(K), d_offsets(), d_targets(), 0, N, AMMSB_ROLES_ALL, 0, 0,
                           d_node() + 3 * N, d_node() + 4 * N, d_node() + 5 * N, d_node() + 6 * N, d_wide(), d_wide() + N,
                           nullptr, nullptr, nullptr, roles, roles + K, roles + 2 * K, roles + 3 * K, stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_roles_nodes", rc, ammsb_roles_last_error());
    std::vector<uint64_t> sums(5 * K + 4);
    std::vector<uint32_t> node(4 * N);
    d_sums.Read(queue_, 5 * K + 4, sums.data());
    d_node.Read(queue_, 4 * N, node.data());
    queue_.Finish();
    r.tri.assign(node.begin(), node.begin() + N);
    r.tri_in.assign(node.begin() + N, node.begin() + 2 * N);
    r.tri_comms.assign(node.begin() + 2 * N, node.begin() + 3 * N);
    r.degree.assign(node.begin() + 3 * N, node.end());
    r.ktri3.assign(sums.begin(), sums.begin() + K);
    r.kpart.assign(sums.begin() + K, sums.begin() + 2 * K);
    const uint64_t* ksum = sums.data() + 2 * K + 2;
    for (uint64_t k = 0; k < K; ++k) {
      r.wedges[k] = (ksum[K + k] - ksum[k]) / 2;
      r.kmembers[k] = ksum[2 * K + k];
    }
    if (sums[2 * K + 1] != 0) throw std::runtime_error("Triangles: the simple adjacency holds a target >= N");
  }
  r.Derive();
}

bool Learner::WriteTriangles(std::ostream* out, Float threshold, const std::vector<Edge>* edges) {
  TrianglesResult r;
  Triangles(threshold, edges, &r);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.M << " " << G9(threshold) << " " << r.skipped << " " << r.dropped
       << " " << r.total << "\n";
  for (size_t k = 0; k < r.ktri3.size(); ++k)
    *out << "c " << k << " " << r.kmembers[k] << " " << r.kpart[k] << " " << r.ktri3[k] << " " << r.wedges[k] << "\n";
  for (size_t a = 0; a < r.degree.size(); ++a)
    *out << "n " << a << " " << r.degree[a] << " " << r.tri[a] << " " << r.tri_in[a] << " " << r.tri_comms[a] << "\n";
  return static_cast<bool>(*out);
}

// ---- is each community one piece: libammsb_components.so over libammsb_connect.so's mask of pi and an edge list
void Learner::ComponentsResult::Derive() {
#pragma STDC FP_CONTRACT OFF
  const size_t K = members.size();
  giant.assign(K, -1.0);
  fragmentation.assign(K, -1.0);
  uint64_t some = 0, whole = 0;
  for (size_t k = 0; k < K; ++k) {
    whole += components[k] == 1;
    if (members[k] == 0) continue;
    ++some;
    // (every integer is converted once, to nearest even)
    giant[k] = static_cast<double>(largest[k]) / static_cast<double>(members[k]);
    fragmentation[k] = 1.0 - giant[k];
  }
  connected = some ? static_cast<double>(whole) / static_cast<double>(some) : -1.0;
}

void Learner::CommunityComponents(Float threshold, ComponentsResult* result, const std::vector<Edge>* edges) {
  CheckThreshold("CommunityComponents", threshold);
  if (edges && edges->size() >= AMMSB_COMPONENTS_MAX_EDGES)
    throw std::invalid_argument("CommunityComponents: an edge list of 2^31 keys or more");
  DrainAsync();
  queue_.Finish();
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  if (K == 0 || K > AMMSB_COMPONENTS_MAX_COLS) throw std::runtime_error("CommunityComponents: K outside 1..8192");
  std::vector<Edge> training;
  edges = EdgesOrTraining("CommunityComponents", edges, cfg_, &training, AMMSB_COMPONENTS_MAX_EDGES);
  ComponentsResult& r = *result;
  r.members.assign(K, 0);
  r.components.assign(K, 0);
  r.singletons.assign(K, 0);
  r.largest.assign(K, 0);
  r.largest_root.assign(K, -1);
  r.offsets.assign(N + 1, 0);
  r.community.clear();
  r.root.clear();
  r.size.clear();
  r.stray.assign(N, 0);
  r.links = r.shared = 0;
  r.skipped = edges->size();  // (without a node every key has an end >= N)
  if (N > 0) {
    const uint32_t cols = static_cast<uint32_t>(K);
    hipStream_t stream = static_cast<hipStream_t>(queue_.stream());
    const clcuda::Context context = queue_.GetContext();
    clcuda::Buffer<uint32_t> d_node(context, 2 * N);  // own, then stray
    const clcuda::Buffer<uint64_t> d_mask = MembershipMask("ammsb_connect_mask", &PostfitPi(), threshold, context, stream);
    int rc = ammsb_components_own(d_mask(), N, cols, d_node(), stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_components_own", rc, ammsb_components_last_error());
    // base: a host prefix sum over the downloaded own
    std::vector<uint32_t> own(N);
    d_node.Read(queue_, N, own.data());
    queue_.Finish();
    for (uint64_t a = 0; a < N; ++a) r.offsets[a + 1] = r.offsets[a] + own[a];
    const uint64_t M = r.offsets[N];
    if (M >= AMMSB_COMPONENTS_MAX_SLOTS)
      throw std::invalid_argument("CommunityComponents: the cover has " + std::to_string(M) + " memberships at the threshold " +
                                  G9(threshold) + "; the library takes fewer than 2^32 (raise the threshold)");
    const uint64_t m1 = std::max<uint64_t>(M, 1);  // (a buffer needs a byte)
    clcuda::Buffer<uint64_t> d_base(context, queue_, r.offsets.begin(), r.offsets.end());
    clcuda::Buffer<uint64_t> d_sums(context, 4 * K + 4);  // members components singletons best; counts
    clcuda::Buffer<uint32_t> d_slot(context, 4 * m1), d_best(context, 2 * K);  // slot_node parent root size; largest largest_root
    clcuda::Buffer<uint16_t> d_comm(context, m1);
    Zero("CommunityComponents", d_sums(), (4 * K + 4) * sizeof(uint64_t), stream);
    uint32_t* const parent = d_slot() + m1;
    uint64_t* const counts = d_sums() + 4 * K;
    if (M > 0) {
      rc = ammsb_components_slots(d_mask(), N, cols, d_base(), M, 0, N, d_slot(), d_comm(), parent, stream);
      if (rc != AMMSB_OK) throw PostfitError("ammsb_components_slots", rc, ammsb_components_last_error());
    }
    if (!edges->empty()) {
      clcuda::Buffer<Edge> d_edges(context, queue_, edges->begin(), edges->end());
      rc = ammsb_components_edges(d_mask(), N, cols, d_base(), M, d_edges(), edges->size(), parent, counts, stream);
      if (rc != AMMSB_OK) throw PostfitError("ammsb_components_edges", rc, ammsb_components_last_error());
      queue_.Finish();  // (the keys' buffer goes out of scope)
    }
    rc = ammsb_components_finish(N, cols, d_base(), M, d_slot(), d_comm(), parent, d_slot() + 2 * m1, d_slot() + 3 * m1, d_sums(),
                                 d_sums() + K, d_sums() + 2 * K, d_sums() + 3 * K, d_best(),
                                 reinterpret_cast<int32_t*>(d_best() + K), d_node() + N, counts, stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_components_finish", rc, ammsb_components_last_error());
    std::vector<uint64_t> sums(4 * K + 4);
    std::vector<uint32_t> best(2 * K), slot(4 * m1), node(2 * N);
    r.community.resize(m1);
    d_sums.Read(queue_, 4 * K + 4, sums.data());
    d_best.Read(queue_, 2 * K, best.data());
    d_slot.Read(queue_, 4 * m1, slot.data());
    d_comm.Read(queue_, m1, r.community.data());
    d_node.Read(queue_, 2 * N, node.data());
    queue_.Finish();
    r.community.resize(M);
    r.root.assign(slot.begin() + 2 * m1, slot.begin() + 2 * m1 + M);
    r.size.assign(slot.begin() + 3 * m1, slot.begin() + 3 * m1 + M);
    r.stray.assign(node.begin() + N, node.end());
    r.members.assign(sums.begin(), sums.begin() + K);
    r.components.assign(sums.begin() + K, sums.begin() + 2 * K);
    r.singletons.assign(sums.begin() + 2 * K, sums.begin() + 3 * K);
    r.largest.assign(best.begin(), best.begin() + K);
    for (uint64_t k = 0; k < K; ++k) r.largest_root[k] = static_cast<int32_t>(best[K + k]);
    r.links = sums[4 * K];
    r.skipped = sums[4 * K + 1];
    r.shared = sums[4 * K + 2];
    if (sums[4 * K + 3] != 0)
      throw std::runtime_error("CommunityComponents: " + std::to_string(sums[4 * K + 3]) +
                               " finds or hooks took more than 2^20 steps and were given up");
  }
  r.Derive();
}

bool Learner::WriteCommunityComponents(std::ostream* out, Float threshold, const std::vector<Edge>* edges) {
  ComponentsResult r;
  CommunityComponents(threshold, &r, edges);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.links + r.skipped << " " << r.root.size() << " " << G9(threshold)
       << " " << r.skipped << " " << r.shared << "\n";
  for (size_t k = 0; k < r.members.size(); ++k)
    *out << "c " << k << " " << r.members[k] << " " << r.components[k] << " " << r.largest[k] << " " << r.largest_root[k] << " "
         << r.singletons[k] << "\n";
  for (size_t a = 0; a + 1 < r.offsets.size(); ++a) {
    *out << "n " << a << " " << r.offsets[a + 1] - r.offsets[a];
    for (uint64_t s = r.offsets[a]; s < r.offsets[a + 1]; ++s) *out << " " << r.community[s] << " " << r.root[s] << " " << r.size[s];
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

// ---- where does a node sit inside a community: libammsb_cores.so over libammsb_connect.so's mask of pi, the slot numbering
// of libammsb_components.so and one simple CSR adjacency
void Learner::CoresResult::Derive() {
#pragma STDC FP_CONTRACT OFF
  const size_t K = members.size(), M = core.size();
  // (every integer is converted once, to nearest even)
  coreness.assign(M, -1.0);
  std::vector<uint64_t> total(K, 0);
  for (size_t s = 0; s < M; ++s) {
    const uint32_t top = degeneracy[community[s]];
    total[community[s]] += core[s];
    if (top > 0) coreness[s] = static_cast<double>(core[s]) / static_cast<double>(top);
  }
  nucleus_share.assign(K, -1.0);
  mean_core.assign(K, -1.0);
  for (size_t k = 0; k < K; ++k) {
    if (members[k] == 0) continue;
    nucleus_share[k] = static_cast<double>(nucleus[k]) / static_cast<double>(members[k]);
    mean_core[k] = static_cast<double>(total[k]) / static_cast<double>(members[k]);
  }
}

void Learner::CommunityCores(Float threshold, CoresResult* result, const std::vector<Edge>* edges, uint64_t max_bytes) {
  CheckThreshold("CommunityCores", threshold);
  DrainAsync();
  queue_.Finish();
  const uint64_t N = pi_->Rows(), K = pi_->Cols();
  if (K == 0 || K > AMMSB_CORES_MAX_COLS) throw std::runtime_error("CommunityCores: K outside 1..8192");
  std::vector<Edge> training;
  const std::vector<Edge>& list = *EdgesOrTraining("CommunityCores", edges, cfg_, &training);
  std::vector<uint64_t> offsets;
  std::vector<Vertex> targets;
  uint64_t valid = 0, lost = 0;
  SimpleAdjacency(list, N, 0, "", &offsets, &targets, &valid, &lost);
  CoresResult& r = *result;
  r = CoresResult();
  r.skipped = lost;
  r.dropped = valid - targets.size() / 2;
  r.members.assign(K, 0);
  r.inlinks2.assign(K, 0);
  r.nucleus.assign(K, 0);
  r.isolated.assign(K, 0);
  r.degeneracy.assign(K, 0);
  r.offsets.assign(N + 1, 0);
  r.best_core.assign(N, 0);
  r.in_nucleus.assign(N, 0);
  r.best_comm.assign(N, -1);
  if (N > 0) {
    const uint32_t cols = static_cast<uint32_t>(K);
    hipStream_t stream = static_cast<hipStream_t>(queue_.stream());
    const clcuda::Context context = queue_.GetContext();
    if (targets.empty()) targets.push_back(0);  // (a buffer needs a byte; no offset reaches it)
    clcuda::Buffer<uint32_t> d_node4(context, 4 * N);  // own best_core best_comm in_nucleus
    uint32_t* const d_node = d_node4();
    const clcuda::Buffer<uint64_t> d_mask = MembershipMask("ammsb_connect_mask", &PostfitPi(), threshold, context, stream);
    int rc = ammsb_components_own(d_mask(), N, cols, d_node, stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_components_own", rc, ammsb_components_last_error());
    std::vector<uint32_t> own(N);
    d_node4.Read(queue_, N, own.data());
    queue_.Finish();
    for (uint64_t a = 0; a < N; ++a) r.offsets[a + 1] = r.offsets[a] + own[a];
    const uint64_t M = r.offsets[N];
    if (M >= AMMSB_CORES_MAX_SLOTS)
      throw std::invalid_argument("CommunityCores: the cover has " + std::to_string(M) + " memberships at the threshold " +
                                  G9(threshold) + "; the library takes fewer than 2^32 (raise the threshold)");
    const uint64_t m1 = std::max<uint64_t>(M, 1);  // (a buffer needs a byte)
    clcuda::Buffer<uint64_t> d_base(context, queue_, r.offsets.begin(), r.offsets.end());
    clcuda::Buffer<uint64_t> d_offsets(context, queue_, offsets.begin(), offsets.end());
    clcuda::Buffer<Vertex> d_targets(context, queue_, targets.begin(), targets.end());
    clcuda::Buffer<uint64_t> d_sums(context, 4 * K + 6);  // members inlinks2 nucleus isolated; counts; tail, next_level
    clcuda::Buffer<uint32_t> d_slot(context, 3 * m1), d_top(context, K);  // slot_node / queue, parent / deg, indeg; degeneracy
    clcuda::Buffer<uint16_t> d_comm(context, m1);
    Zero("CommunityCores", d_sums(), (4 * K + 6) * sizeof(uint64_t), stream);
    Zero("CommunityCores", d_top(), K * sizeof(uint32_t), stream);
    uint64_t* const counts = d_sums() + 4 * K;
    uint64_t* const tail_p = counts + 4;
    uint32_t* const next_p = reinterpret_cast<uint32_t*>(counts + 5);
    uint32_t* const queue = d_slot();      // (slot_node and parent are only there for ammsb_components_slots to write)
    uint32_t* const deg = d_slot() + m1;
    uint32_t* const indeg = d_slot() + 2 * m1;
    std::vector<uint32_t> h_indeg(m1, 0);
    if (M > 0) {
      rc = ammsb_components_slots(d_mask(), N, cols, d_base(), M, 0, N, queue, d_comm(), deg, stream);
      if (rc != AMMSB_OK) throw PostfitError("ammsb_components_slots", rc, ammsb_components_last_error());
      rc = ammsb_cores_degrees(d_mask(), N, cols, d_base(), M, d_offsets(), d_targets(), 0, N, indeg, counts, stream);
      if (rc != AMMSB_OK) throw PostfitError("ammsb_cores_degrees", rc, ammsb_cores_last_error());
      // nbr_off: a host prefix sum over the downloaded indeg
      if (hipMemcpyAsync(h_indeg.data(), indeg, M * sizeof(uint32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess)
        throw std::runtime_error("CommunityCores: reading the inner degrees back failed");
      std::vector<uint64_t> nbr_off(M + 1, 0);
      for (uint64_t s = 0; s < M; ++s) nbr_off[s + 1] = nbr_off[s] + h_indeg[s];
      r.L = nbr_off[M];
      if (r.L >= AMMSB_CORES_MAX_NBR || 4 * r.L > max_bytes)
        throw std::invalid_argument("CommunityCores: the induced subgraphs hold " + std::to_string(r.L) +
                                    " neighbour entries at the threshold " + G9(threshold) + ", " + std::to_string(4 * r.L) +
                                    " bytes; the library takes fewer than 2^32 entries and max_bytes is " +
                                    std::to_string(max_bytes) + " (raise the threshold)");
      clcuda::Buffer<uint64_t> d_nbr_off(context, queue_, nbr_off.begin(), nbr_off.end());
      clcuda::Buffer<uint32_t> d_nbr(context, std::max<uint64_t>(r.L, 1));
      rc = ammsb_cores_adjacency(d_mask(), N, cols, d_base(), M, d_offsets(), d_targets(), 0, N, indeg, d_nbr_off(), r.L, d_nbr(),
                                 stream);
      if (rc != AMMSB_OK) throw PostfitError("ammsb_cores_adjacency", rc, ammsb_cores_last_error());
      if (hipMemcpyAsync(deg, indeg, M * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream) != hipSuccess)
        throw std::runtime_error("CommunityCores: copying the inner degrees failed");
      // the host loop of the header: 12 bytes back after every launch, at most M peel launches
      struct {
        uint64_t tail;
        uint32_t next;
      } ctl = {0, 0};
      const auto read = [&]() {
        if (hipMemcpyAsync(&ctl, tail_p, 12, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
          throw std::runtime_error("CommunityCores: reading the queue's tail back failed");
      };
      uint64_t head = 0;
      uint32_t level = 0;
      const uint32_t none = 0xFFFFFFFFu;
      for (;;) {
        if (hipMemcpyAsync(next_p, &none, 4, hipMemcpyHostToDevice, stream) != hipSuccess)
          throw std::runtime_error("CommunityCores: resetting next_level failed");
        rc = ammsb_cores_scan(M, level, deg, queue, tail_p, next_p, counts, stream);
        if (rc != AMMSB_OK) throw PostfitError("ammsb_cores_scan", rc, ammsb_cores_last_error());
        read();
        if (ctl.tail == head) {  // nothing at this level
          if (ctl.tail >= M || ctl.next == none) break;
          level = ctl.next;  // (no peel ran since the scan: the smallest degree left)
          continue;
        }
        if (level == 0) head = ctl.tail;  // (a slot of degree 0 has no row: nothing to lower)
        while (head < ctl.tail) {
          rc = ammsb_cores_peel(M, level, head, ctl.tail, d_nbr_off(), indeg, d_nbr(), r.L, deg, queue, tail_p, counts, stream);
          if (rc != AMMSB_OK) throw PostfitError("ammsb_cores_peel", rc, ammsb_cores_last_error());
          head = ctl.tail;
          read();
          if (ctl.tail > M) throw std::runtime_error("CommunityCores: the queue holds more slots than there are");
        }
        if (ctl.tail >= M) break;
        ++level;
      }
      if (ctl.tail != M) throw std::runtime_error("CommunityCores: the peel ended before every slot was queued");
    }
    rc = ammsb_cores_finish(N, cols, d_base(), M, d_comm(), indeg, deg, d_sums(), d_sums() + K, d_top(), d_sums() + 2 * K,
                            d_sums() + 3 * K, d_node + N, reinterpret_cast<int32_t*>(d_node + 2 * N), d_node + 3 * N,
                            stream);
    if (rc != AMMSB_OK) throw PostfitError("ammsb_cores_finish", rc, ammsb_cores_last_error());
    std::vector<uint64_t> sums(4 * K + 6);
    std::vector<uint32_t> slot(3 * m1), node(4 * N);
    r.community.resize(m1);
    r.degeneracy.resize(K);
    d_sums.Read(queue_, 4 * K + 6, sums.data());
    d_top.Read(queue_, K, r.degeneracy.data());
    d_slot.Read(queue_, 3 * m1, slot.data());
    d_comm.Read(queue_, m1, r.community.data());
    d_node4.Read(queue_, 4 * N, node.data());
    queue_.Finish();
    r.community.resize(M);
    r.core.assign(slot.begin() + m1, slot.begin() + m1 + M);
    r.indeg.assign(slot.begin() + 2 * m1, slot.begin() + 2 * m1 + M);
    r.best_core.assign(node.begin() + N, node.begin() + 2 * N);
    for (uint64_t a = 0; a < N; ++a) r.best_comm[a] = static_cast<int32_t>(node[2 * N + a]);
    r.in_nucleus.assign(node.begin() + 3 * N, node.end());
    r.members.assign(sums.begin(), sums.begin() + K);
    r.inlinks2.assign(sums.begin() + K, sums.begin() + 2 * K);
    r.nucleus.assign(sums.begin() + 2 * K, sums.begin() + 3 * K);
    r.isolated.assign(sums.begin() + 3 * K, sums.begin() + 4 * K);
    if (sums[4 * K] != M || sums[4 * K + 1] != r.L) throw std::runtime_error("CommunityCores: the device's counts contradict the arrays");
    r.scans = sums[4 * K + 2];
    r.rounds = sums[4 * K + 3];
  }
  r.Derive();
}

bool Learner::WriteCommunityCores(std::ostream* out, Float threshold, const std::vector<Edge>* edges) {
  CoresResult r;
  CommunityCores(threshold, &r, edges);
  *out << "# " << pi_->Rows() << " " << pi_->Cols() << " " << r.core.size() << " " << r.L << " " << G9(threshold) << " " << r.skipped
       << " " << r.dropped << "\n";
  for (size_t k = 0; k < r.members.size(); ++k)
    *out << "c " << k << " " << r.members[k] << " " << r.inlinks2[k] << " " << r.degeneracy[k] << " " << r.nucleus[k] << " "
         << r.isolated[k] << "\n";
  for (size_t a = 0; a + 1 < r.offsets.size(); ++a) {
    *out << "n " << a << " " << r.offsets[a + 1] - r.offsets[a];
    for (uint64_t s = r.offsets[a]; s < r.offsets[a + 1]; ++s) *out << " " << r.community[s] << " " << r.indeg[s] << " " << r.core[s];
    *out << "\n";
  }
  return static_cast<bool>(*out);
}

}  // namespace mcmc
