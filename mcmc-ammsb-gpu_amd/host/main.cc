// Command-line driver with the reference's flags and flow (main.cc:26-172): load a SNAP edge list
// (or a gzip data-set dump), split off the held-out set, build the Learner, alternate Run(ppx_interval)
// with HeldoutPerplexity() until max-iters or SIGINT, print the statistics.
// boost::program_options is replaced by a small table-driven parser accepting the same spellings
// (--name value, --name=value, -x value).  New flags are marked (new).
#include <signal.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "mcmc/data.h"
#include "mcmc/exchange.h"
#include "mcmc/learner.h"

namespace clcuda = mcmc::clcuda;

namespace {

sig_atomic_t signaled = 0;
void handler(int) { signaled = 1; }

struct Option {
  std::string name;  // long name
  char shorthand;    // 0 if none
  std::string help;  // default value as text
  std::function<bool(const std::string&)> set;
};

template <class T>
Option Opt(const std::string& name, char s, T* target, const std::string& def) {
  return Option{name, s, def, [target](const std::string& v) {
                  try {  // (the enum / pair parsers throw on a bad token: config.cc:118-131)
                    std::istringstream in(v);
                    in >> std::boolalpha >> *target;
                    if (in.fail()) {  // bool also accepts 0/1, as program_options does
                      std::istringstream again(v);
                      again >> *target;
                      return !again.fail();
                    }
                    return true;
                  } catch (const std::exception&) {
                    return false;
                  }
                }};
}

Option OptStr(const std::string& name, char s, std::string* target) {
  return Option{name, s, "", [target](const std::string& v) {
                  *target = v;
                  return true;
                }};
}

bool FileExists(const std::string& f) {
  std::ifstream in(f);
  return in.good();
}

[[noreturn]] void Fatal(const std::string& msg) {
  std::cerr << "F " << msg << std::endl;
  exit(2);
}

}  // namespace

int main(int argc, char** argv) {
  {
    std::ostringstream s;
    for (int i = 0; i < argc; ++i) s << argv[i] << " ";
    std::cerr << "I " << s.str() << std::endl;
  }
  std::string filename, loadFile, dumpFile, ckptIn, ckptOut, exchangeKind, communitiesOut, linksOut, linksNodes, linksExclude, linkCommOut, qualityOut, groundTruth, coverMatchOut, coverNmiOut, coverOmegaOut, coverOmegaUniverse, relatedOut, relatedBy, linkedOut, linkedBy, modularityOut, rolesOut, rolesAmong = "all", trianglesOut;
  bool haveCoverThreshold = false;
  double coverThreshold = 0.05;
  bool haveRelatedThreshold = false, haveRelatedTop = false;
  double relatedThreshold = 0.05;
  long relatedTop = 4;
  bool haveLinkedThreshold = false, haveLinkedTop = false, haveLinkedMinLinks = false;
  double linkedThreshold = 0.05;
  long linkedTop = 4;
  long long linkedMinLinks = 1;
  bool haveModularityThreshold = false;
  double modularityThreshold = 0.05;
  bool haveRolesThreshold = false, haveRolesTop = false, haveRolesAmong = false;
  double rolesThreshold = 0.05;
  long rolesTop = 4;
  bool haveTrianglesThreshold = false;
  double trianglesThreshold = 0.05;
  bool haveQualityThreshold = false;
  double qualityThreshold = 0.05;
  bool haveLinkCommTop = false, haveLinkCommMinTerm = false;
  long linkCommTop = 1;
  double linkCommMinTerm = 0;
  bool haveLinksTop = false;
  long linksTop = 10;
  bool haveMembershipTop = false, haveMembershipThreshold = false;
  long membershipTop = 4;
  double membershipThreshold = 0;
  int deviceId = -1;
  mcmc::Config cfg;
  uint32_t max_iters = 100;
  bool dumpDataset = false, loadDataset = false;
  cfg.alpha = 0;            // main.cc:50
  cfg.beta_seed = {44, 45};  // main.cc:69-70 (the struct defaults differ)
  cfg.neighbor_seed = {56, 57};
  std::vector<Option> options = {
      OptStr("file", 'f', &filename),
      Opt("train-ppx-ratio", 0, &cfg.training_ppx_ratio, "0.01"),  // main.cc:47-49 (MCMC_CALC_TRAIN_PPX builds)
      Opt("train-ppx", 0, &cfg.calc_train_ppx, "0 (new: the reference's MCMC_CALC_TRAIN_PPX build option at run time)"),
      Opt("heldout-ratio", 'r', &cfg.heldout_ratio, "0.01"),
      Opt("alpha", 0, &cfg.alpha, "0"),
      Opt("a", 'a', &cfg.a, "0.0315"),
      Opt("b", 'b', &cfg.b, "1024"),
      Opt("c", 'c', &cfg.c, "0.5"),
      Opt("epsilon", 'e', &cfg.epsilon, "1e-07"),
      Opt("eta0", 0, &cfg.eta0, "1"),
      Opt("eta1", 0, &cfg.eta1, "1"),
      Opt("k", 'k', &cfg.K, "32"),
      Opt("mini_batch", 'm', &cfg.mini_batch_size, "32"),
      Opt("neighbors", 'n', &cfg.num_node_sample, "32"),
      Opt("ppx-wg", 0, &cfg.ppx_wg_size, "32"),
      Opt("ppx-interval", 'i', &cfg.ppx_interval, "100"),
      Opt("phi-wg", 0, &cfg.phi_wg_size, "32"),
      Opt("beta-wg", 0, &cfg.beta_wg_size, "32"),
      Opt("max-iters", 'x', &max_iters, "100"),
      Opt("sample", 's', &cfg.strategy, "Node"),
      Opt("sampler-wg", 0, &cfg.neighbor_sampler_wg_size, "32"),
      Opt("phi-seed", 0, &cfg.phi_seed, "42,43"),
      Opt("beta-seed", 0, &cfg.beta_seed, "44,45"),
      Opt("neighbor-seed", 0, &cfg.neighbor_seed, "56,57"),
      Opt("phi-mode", 0, &cfg.phi_mode, "PHI_NODE_PER_WORKGROUP_NAIVE"),
      Opt("phi-probs-shared", 0, &cfg.phi_probs_shared, "1"),
      Opt("phi-grads-shared", 0, &cfg.phi_grads_shared, "1"),
      Opt("phi-pi-shared", 0, &cfg.phi_pi_shared, "1"),
      Opt("phi-vwidth", 0, &cfg.phi_vector_width, "1"),
      Opt("beta-sum-grads-vwidth", 0, &cfg.sum_grads_vector_width, "1"),
      Opt("dump-data", 0, &dumpDataset, "0"),
      OptStr("dump-file", 0, &dumpFile),
      Opt("load-data", 0, &loadDataset, "0"),
      OptStr("load-file", 0, &loadFile),
      Opt("phi-disable-noise", 0, &cfg.phi_disable_noise, "0 (new)"),
      Opt("sample-seed0", 0, &cfg.sample_seed[0], "1804289383 (new: rand_r seeds of the two sample buffers)"),
      Opt("sample-seed1", 0, &cfg.sample_seed[1], "846930886 (new)"),
      Opt("device-sampling", 0, &cfg.device_sampling, "0 (new: draw mini-batches on the device)"),
      Option{"sampling-stream", 0,
             "own (new, with --device-sampling 1: own | reference; reference = the reference's rand_r stream and "
             "unordered_set orders drawn on the device from --sample-seed0/1, host sampling's mini-batches bit for bit; "
             "not with --graph 1)",
             [&cfg](const std::string& v) {
               cfg.sampling_stream = v;
               return v == "own" || v == "reference";
             }},
      Opt("async", 0, &cfg.async_launch, "0 (new: enqueue-only loop; needs --device-sampling 1)"),
      Opt("graph", 0, &cfg.graph_launch, "0 (new: iterations as captured hipGraphs; needs --async 1)"),
      Opt("loop-timers", 0, &cfg.loop_timers, "1 (new: per-kernel device times in PrintStats under --async / --graph)"),
      Opt("phi-chunks", 0, &cfg.phi_chunks, "4 (new, with --exchange: blocks per rank whose exchange overlaps the next block's update_phi)"),
      Opt("phi-replicate", 0, &cfg.phi_replicate, "-1 (new, with --exchange: fraction of the virtual groups every rank computes itself; < 0 = measured at start-up)"),
      Opt("pi-candidates", 0, &cfg.pi_placement_candidates, "12 (new: allocations of pi timed under update_phi at start-up, the fastest kept; 0 = off)"),
      Opt("beta-grads", 0, &cfg.beta_grads, "-1 (new, with --exchange: 0 = gradient cut over the ranks + all-gather, 1 = every rank the whole gradient, -1 = 1 where update_pi folds into its launch)"),
      Opt("beta-shard-min-edges", 0, &cfg.beta_shard_min_edges, "4096 (new, with --exchange: mini-batches of at most this many edges keep their whole gradient on every rank)"),
      OptStr("exchange", 0, &exchangeKind),  // (new) rccl | host: one process per GPU, RANK / WORLD_SIZE / MASTER_* from the env
      Opt("device", 0, &deviceId, "-1 (new: HIP device; default LOCAL_RANK with --exchange, else 0)"),
      OptStr("checkpoint-in", 0, &ckptIn),    // (new) Learner::Parse before the first iteration
      OptStr("checkpoint-out", 0, &ckptOut),  // (new) Learner::Serialize after the last one
      OptStr("communities-out", 0, &communitiesOut),  // (new) after the last perplexity line: `# N K top threshold`, then `k size n0 n1 ...` per community
      OptStr("link-communities-out", 0, &linkCommOut),  // (new) after the last perplexity line: `# N K E top min_term`, then `a b p n k0 t0 k1 t1 ...` per training link
      Option{"link-communities-top", 0, "1 (new, with --link-communities-out: largest terms kept per link, 1..16)",
             [&](const std::string& v) {
               haveLinkCommTop = true;
               std::istringstream in(v);
               in >> linkCommTop;
               return !in.fail() && in.eof();
             }},
      Option{"link-communities-min-term", 0, "0 (new, with --link-communities-out: terms below it take no slot)",
             [&](const std::string& v) {
               haveLinkCommMinTerm = true;
               std::istringstream in(v);
               in >> linkCommMinTerm;
               return !in.fail() && in.eof();
             }},
      OptStr("community-quality-out", 0, &qualityOut),  // (new) after the last perplexity line: `# N K E threshold uncovered`, then `k size internal boundary conductance density` per community
      Option{"community-quality-threshold", 0, "0.05 (new, with --community-quality-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveQualityThreshold = true;
               std::istringstream in(v);
               in >> qualityThreshold;
               return !in.fail() && in.eof();
             }},
      OptStr("ground-truth", 0, &groundTruth),  // (new, with --cover-match-out) a SNAP cmty file: one community per line; the graph file's own ids with --file, dense ids with --load-data
      OptStr("cover-match-out", 0, &coverMatchOut),  // (new, with --ground-truth) after the last perplexity line: `# N K G threshold skipped f1_truth f1_detected avg_f1`, then `t g size best overlap f1` per ground-truth and `d k size best overlap f1` per detected community
      OptStr("cover-nmi-out", 0, &coverNmiOut),  // (new, with --ground-truth) after the last perplexity line: `# N K G threshold skipped nmi_lfk nmi_max`, then `t g size H h` per ground-truth and `d k size H h` per detected community (H the entropy, h the conditional entropy given the other cover; %.17g)
      OptStr("cover-omega-out", 0, &coverOmegaOut),  // (new, with --ground-truth) after the last perplexity line: `# N K G threshold universe_n skipped outside omega omega_unadjusted`, then `j agree detected truth` per level: the pairs of the universe that share j communities (%.17g, `nan` where undefined)
      OptStr("cover-omega-universe", 0, &coverOmegaUniverse),  // (new, with --cover-omega-out) covered (default: the nodes some ground-truth community holds) | all
      Option{"cover-match-threshold", 0, "0.05 (new, with --ground-truth and --cover-match-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveCoverThreshold = true;
               std::istringstream in(v);
               in >> coverThreshold;
               return !in.fail() && in.eof();
             }},
      OptStr("related-communities-out", 0, &relatedOut),  // (new) after the last perplexity line: `# N K threshold by top min_overlap`, then `k size n l0 o0 l1 o1 ...` per community: its n closest other communities and the nodes it shares with each
      Option{"related-communities-threshold", 0, "0.05 (new, with --related-communities-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveRelatedThreshold = true;
               std::istringstream in(v);
               in >> relatedThreshold;
               return !in.fail() && in.eof();
             }},
      Option{"related-communities-top", 0, "4 (new, with --related-communities-out: closest communities kept per community, 1..64)",
             [&](const std::string& v) {
               haveRelatedTop = true;
               std::istringstream in(v);
               in >> relatedTop;
               return !in.fail() && in.eof();
             }},
      OptStr("related-communities-by", 0, &relatedBy),  // (new, with --related-communities-out) jaccard (default) | overlap | contained
      OptStr("linked-communities-out", 0, &linkedOut),  // (new) after the last perplexity line: `# N K E threshold by top min_links skipped`, then `k size internal n l0 w0 o0 l1 w1 o1 ...` per community: the n other communities it is linked to most, the training links to each and the nodes shared with each
      Option{"linked-communities-threshold", 0, "0.05 (new, with --linked-communities-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveLinkedThreshold = true;
               std::istringstream in(v);
               in >> linkedThreshold;
               return !in.fail() && in.eof();
             }},
      Option{"linked-communities-top", 0, "4 (new, with --linked-communities-out: partners kept per community, 1..64)",
             [&](const std::string& v) {
               haveLinkedTop = true;
               std::istringstream in(v);
               in >> linkedTop;
               return !in.fail() && in.eof();
             }},
      OptStr("linked-communities-by", 0, &linkedBy),  // (new, with --linked-communities-out) density (default) | links
      Option{"linked-communities-min-links", 0, "1 (new, with --linked-communities-out: fewest links that make a partner)",
             [&](const std::string& v) {
               haveLinkedMinLinks = true;
               std::istringstream in(v);
               in >> linkedMinLinks;
               return !in.fail() && in.eof();
             }},
      OptStr("modularity-out", 0, &modularityOut),  // (new) after the last perplexity line: `# N K E threshold skipped q`, then `k q_k in_k s_k internal volume` per community: the overlapping modularity of the cover against the training links, the 128-bit sums as 32 hexadecimal digits
      Option{"modularity-threshold", 0, "0.05 (new, with --modularity-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveModularityThreshold = true;
               std::istringstream in(v);
               in >> modularityThreshold;
               return !in.fail() && in.eof();
             }},
      OptStr("node-roles-out", 0, &rolesOut),  // (new) after the last perplexity line: `# N K M threshold among top min_count skipped`, `c k members ksum ksq` per community, `n a degree own embedded reached votes squares nslots k0 c0 f0 ...` per node: how each node sits in the cover against the training adjacency
      Option{"node-roles-threshold", 0, "0.05 (new, with --node-roles-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveRolesThreshold = true;
               std::istringstream in(v);
               in >> rolesThreshold;
               return !in.fail() && in.eof();
             }},
      Option{"node-roles-top", 0, "4 (new, with --node-roles-out: communities kept per node, 1..16)",
             [&](const std::string& v) {
               haveRolesTop = true;
               std::istringstream in(v);
               in >> rolesTop;
               return !in.fail() && in.eof();
             }},
      Option{"node-roles-among", 0, "all (new, with --node-roles-out: all = every community a neighbour is in, own = the node's own)",
             [&](const std::string& v) {
               haveRolesAmong = true;
               rolesAmong = v;
               return true;
             }},
      OptStr("triangles-out", 0, &trianglesOut),  // (new) after the last perplexity line: `# N K M threshold skipped dropped total`, `c k members part tri3 wedges` per community, `n a degree tri tri_in tri_comms` per node: the triangles of the training adjacency inside the detected communities
      Option{"triangles-threshold", 0, "0.05 (new, with --triangles-out: a node is a member of k iff pi[a, k] >= it)",
             [&](const std::string& v) {
               haveTrianglesThreshold = true;
               std::istringstream in(v);
               in >> trianglesThreshold;
               return !in.fail() && in.eof();
             }},
      OptStr("links-out", 0, &linksOut),      // (new) after the last perplexity line: `# N K top exclude`, then `a n b0 s0 b1 s1 ...` per query node
      Option{"links-top", 0, "10 (new, with --links-out: most probable partners kept per node, 1..64)",
             [&](const std::string& v) {
               haveLinksTop = true;
               std::istringstream in(v);
               in >> linksTop;
               return !in.fail() && in.eof();
             }},
      OptStr("links-nodes", 0, &linksNodes),      // (new, with --links-out) file of query node ids; default: every node
      OptStr("links-exclude", 0, &linksExclude),  // (new, with --links-out) none | training | all (default: training and held-out edges)
      Option{"membership-top", 0, "4 (new, with --communities-out: strongest communities kept per node, 1..16)",
             [&](const std::string& v) {
               haveMembershipTop = true;
               std::istringstream in(v);
               in >> membershipTop;
               return !in.fail() && in.eof();
             }},
      Option{"membership-threshold", 0, "0 (new, with --communities-out: a node is a member where pi >= this)",
             [&](const std::string& v) {
               haveMembershipThreshold = true;
               std::istringstream in(v);
               in >> membershipThreshold;
               return !in.fail() && in.eof();
             }},
  };
  for (int i = 1; i < argc; ++i) {
    std::string arg = argv[i], value;
    if (arg == "--help" || arg == "-h") {
      for (const Option& o : options) {
        std::cout << "  ";
        if (o.shorthand) std::cout << "-" << o.shorthand << " [ --" << o.name << " ]";
        else std::cout << "--" << o.name;
        std::cout << " arg";
        if (!o.help.empty()) std::cout << " (=" << o.help << ")";
        std::cout << "\n";
      }
      return 1;  // main.cc:86-89
    }
    const Option* opt = nullptr;
    bool have_value = false;
    if (arg.rfind("--", 0) == 0) {
      const size_t eq = arg.find('=');
      const std::string name = arg.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
      for (const Option& o : options)
        if (o.name == name) opt = &o;
      if (eq != std::string::npos) {
        value = arg.substr(eq + 1);
        have_value = true;
      }
    } else if (arg.size() >= 2 && arg[0] == '-') {
      for (const Option& o : options)
        if (o.shorthand && o.shorthand == arg[1]) opt = &o;
      if (arg.size() > 2) {
        value = arg.substr(2);
        have_value = true;
      }
    }
    if (!opt) Fatal("unrecognised option '" + arg + "'");
    if (!have_value) {
      if (i + 1 >= argc) Fatal("the required argument for option '" + arg + "' is missing");
      value = argv[++i];
    }
    if (!opt->set(value)) Fatal("the argument ('" + value + "') for option '--" + opt->name + "' is invalid");
  }
  if (cfg.sampling_stream == "reference" && cfg.graph_launch)
    Fatal("--sampling-stream reference cannot be combined with --graph 1: the descriptor loop needs each mini-batch's "
          "sizes before the device has drawn it (use --async 1 without --graph, or the synchronous loop)");
  if (cfg.sampling_stream == "reference" && !cfg.device_sampling)
    Fatal("--sampling-stream reference needs --device-sampling 1 (without it the host samplers draw that same stream)");
  if ((haveMembershipTop || haveMembershipThreshold) && communitiesOut.empty())
    Fatal("--membership-top / --membership-threshold need --communities-out FILE");
  if (membershipTop < 1 || membershipTop > 16) Fatal("--membership-top must be in 1..16");
  if (!(membershipThreshold >= 0)) Fatal("--membership-threshold must be >= 0");
  if ((haveLinkCommTop || haveLinkCommMinTerm) && linkCommOut.empty())
    Fatal("--link-communities-top / --link-communities-min-term need --link-communities-out FILE");
  if (linkCommTop < 1 || linkCommTop > 16) Fatal("--link-communities-top must be in 1..16");
  if (!(linkCommMinTerm >= 0) || !std::isfinite(static_cast<float>(linkCommMinTerm)))
    Fatal("--link-communities-min-term must be finite and >= 0");
  if (haveQualityThreshold && qualityOut.empty()) Fatal("--community-quality-threshold needs --community-quality-out FILE");
  if (!(qualityThreshold >= 0) || !std::isfinite(static_cast<float>(qualityThreshold)))
    Fatal("--community-quality-threshold must be finite and >= 0");
  if (groundTruth.empty() && !coverMatchOut.empty()) Fatal("--ground-truth FILE and --cover-match-out FILE need each other");
  if (groundTruth.empty() && !coverNmiOut.empty()) Fatal("--cover-nmi-out FILE needs --ground-truth FILE");
  if (groundTruth.empty() && !coverOmegaOut.empty()) Fatal("--cover-omega-out FILE needs --ground-truth FILE");
  if (!groundTruth.empty() && coverMatchOut.empty() && coverNmiOut.empty() && coverOmegaOut.empty())
    Fatal("--ground-truth FILE and --cover-match-out FILE need each other (or --cover-nmi-out FILE, or --cover-omega-out FILE)");
  if (haveCoverThreshold && coverMatchOut.empty() && coverNmiOut.empty() && coverOmegaOut.empty())
    Fatal("--cover-match-threshold needs --ground-truth FILE and --cover-match-out FILE (or --cover-nmi-out FILE, or --cover-omega-out FILE)");
  if (!coverOmegaUniverse.empty() && coverOmegaOut.empty()) Fatal("--cover-omega-universe needs --cover-omega-out FILE");
  if (!coverOmegaUniverse.empty() && coverOmegaUniverse != "covered" && coverOmegaUniverse != "all")
    Fatal("--cover-omega-universe must be covered or all");
  if (!(coverThreshold >= 0) || !std::isfinite(static_cast<float>(coverThreshold)))
    Fatal("--cover-match-threshold must be finite and >= 0");
  if ((haveRelatedThreshold || haveRelatedTop || !relatedBy.empty()) && relatedOut.empty())
    Fatal("--related-communities-threshold / --related-communities-top / --related-communities-by need --related-communities-out FILE");
  if (!relatedBy.empty() && relatedBy != "jaccard" && relatedBy != "overlap" && relatedBy != "contained")
    Fatal("--related-communities-by must be jaccard, overlap or contained");
  if (relatedTop < 1 || relatedTop > 64) Fatal("--related-communities-top must be in 1..64");
  if (!(relatedThreshold >= 0) || !std::isfinite(static_cast<float>(relatedThreshold)))
    Fatal("--related-communities-threshold must be finite and >= 0");
  if ((haveLinkedThreshold || haveLinkedTop || haveLinkedMinLinks || !linkedBy.empty()) && linkedOut.empty())
    Fatal("--linked-communities-threshold / --linked-communities-top / --linked-communities-by / --linked-communities-min-links need --linked-communities-out FILE");
  if (!linkedBy.empty() && linkedBy != "density" && linkedBy != "links")
    Fatal("--linked-communities-by must be density or links");
  if (linkedTop < 1 || linkedTop > 64) Fatal("--linked-communities-top must be in 1..64");
  if (!(linkedThreshold >= 0) || !std::isfinite(static_cast<float>(linkedThreshold)))
    Fatal("--linked-communities-threshold must be finite and >= 0");
  if (linkedMinLinks < 0) Fatal("--linked-communities-min-links must be >= 0");
  if (haveModularityThreshold && modularityOut.empty()) Fatal("--modularity-threshold needs --modularity-out FILE");
  if (!(modularityThreshold >= 0) || !std::isfinite(static_cast<float>(modularityThreshold)))
    Fatal("--modularity-threshold must be finite and >= 0");
  if ((haveRolesThreshold || haveRolesTop || haveRolesAmong) && rolesOut.empty())
    Fatal("--node-roles-threshold / --node-roles-top / --node-roles-among need --node-roles-out FILE");
  if (!(rolesThreshold >= 0) || !std::isfinite(static_cast<float>(rolesThreshold)))
    Fatal("--node-roles-threshold must be finite and >= 0");
  if (rolesTop < 1 || rolesTop > 16) Fatal("--node-roles-top must be in 1..16");
  if (rolesAmong != "all" && rolesAmong != "own") Fatal("--node-roles-among must be all or own");
  if (haveTrianglesThreshold && trianglesOut.empty()) Fatal("--triangles-threshold needs --triangles-out FILE");
  if (!(trianglesThreshold >= 0) || !std::isfinite(static_cast<float>(trianglesThreshold)))
    Fatal("--triangles-threshold must be finite and >= 0");
  if ((haveLinksTop || !linksNodes.empty() || !linksExclude.empty()) && linksOut.empty())
    Fatal("--links-top / --links-nodes / --links-exclude need --links-out FILE");
  if (linksTop < 1 || linksTop > 64) Fatal("--links-top must be in 1..64");
  uint32_t linksMask = mcmc::Learner::kExcludeTraining | mcmc::Learner::kExcludeHeldout;
  if (linksExclude == "none") linksMask = 0;
  else if (linksExclude == "training") linksMask = mcmc::Learner::kExcludeTraining;
  else if (!linksExclude.empty() && linksExclude != "all") Fatal("--links-exclude must be none, training or all");
  std::vector<mcmc::Vertex> linkNodes;
  if (!linksNodes.empty()) {
    std::ifstream in(linksNodes);
    if (!in.good()) Fatal("cannot read --links-nodes file " + linksNodes);
    unsigned long long v;
    while (in >> v) {
      if (v > 0xFFFFFFFFull) Fatal("--links-nodes: node id " + std::to_string(v) + " is not a node id");
      linkNodes.push_back(static_cast<mcmc::Vertex>(v));
    }
    if (!in.eof()) Fatal("--links-nodes: " + linksNodes + " holds something that is not a node id");
  }
  if (!loadDataset && !FileExists(filename)) Fatal("Failed to detect file: " + filename);  // main.cc:91-96
  if (loadDataset && loadFile.empty()) Fatal("load-file is required with load-data");
  if (dumpDataset && dumpFile.empty()) Fatal("dump-file is required with dump-data");

  std::vector<mcmc::Edge> unique_edges;
  std::vector<mcmc::Vertex> originalIds;  // of a text graph: the file's id of every dense id
  if (!loadDataset) {
    if (!mcmc::GetUniqueEdgesFromFile(filename, &cfg.N, &unique_edges, &originalIds)) Fatal("Failed to generate sets from file " + filename);
    if (dumpDataset) {  // main.cc:110-127: dump and stop
      if (!mcmc::DumpDataset(dumpFile, cfg.N, cfg.heldout_ratio, unique_edges)) Fatal("cannot write " + dumpFile);
      return 0;
    }
  } else if (!mcmc::LoadDataset(loadFile, &cfg.N, &cfg.heldout_ratio, &unique_edges)) {
    Fatal("cannot read " + loadFile);
  }
  if (!mcmc::GenerateSetsFromEdges(cfg.N, unique_edges, cfg.heldout_ratio, &cfg.training_edges, &cfg.heldout_edges,
                                   &cfg.training, &cfg.heldout))
    Fatal("Failed to generate training/heldout sets");
  std::vector<uint64_t> truthOffsets;
  std::vector<uint32_t> truthMembers;
  if (!groundTruth.empty()) {
    // a text graph's ground truth speaks of the graph file's own ids, a data-set dump's of dense ids
    uint64_t dropped = 0;
    if (!mcmc::ReadCover(groundTruth, loadDataset ? nullptr : &originalIds, &truthOffsets, &truthMembers, &dropped))
      Fatal("cannot read --ground-truth file " + groundTruth);
    std::cerr << "I ground truth " << groundTruth << ": " << truthOffsets.size() - 1 << " communities, "
              << truthMembers.size() << " members, " << dropped << " ids the graph never mentions dropped" << std::endl;
  }
  for (mcmc::Vertex v : linkNodes)
    if (v >= cfg.N) Fatal("--links-nodes: node id " + std::to_string(v) + " >= N = " + std::to_string(cfg.N));
  cfg.trainingGraph.reset(new mcmc::Graph(cfg.N, cfg.training_edges));
  cfg.heldoutGraph.reset(new mcmc::Graph(cfg.N, cfg.heldout_edges));
  if (cfg.alpha == 0) cfg.alpha = static_cast<mcmc::Float>(1) / cfg.K;  // main.cc:153
  cfg.E = unique_edges.size();

  if (deviceId < 0) {
    const char* lr = exchangeKind.empty() ? nullptr : getenv("LOCAL_RANK");
    deviceId = lr ? atoi(lr) : 0;
  }
  clcuda::Platform platform((size_t)0);
  clcuda::Device dev(platform, static_cast<size_t>(deviceId));
  clcuda::Context context(dev);
  clcuda::Queue queue(context, dev);
  int rank = 0;
  if (!exchangeKind.empty()) {
    try {
      cfg.exchange = mcmc::Exchange::FromEnvironment(exchangeKind, deviceId);
    } catch (const std::exception& e) {
      Fatal(std::string("exchange: ") + e.what());
    }
    rank = cfg.exchange->rank();
    std::cerr << "I exchange " << cfg.exchange->kind() << ": rank " << rank << " of " << cfg.exchange->world()
              << " on device " << deviceId << std::endl;
  }
  std::cerr << "I HIP:\n  Platform: " << dev.Vendor() << "\n  Device: " << dev.Name()
            << "\n  Device Driver: " << dev.Version() << std::endl;
  std::cerr << "I Loaded file " << (loadDataset ? loadFile : filename)
            << " (training max fan out = " << cfg.trainingGraph->MaxFanOut()
            << ", heldout max fan out = " << cfg.heldoutGraph->MaxFanOut() << ")" << std::endl;
  std::cerr << "I " << cfg << std::endl;
  signal(SIGINT, handler);
  std::unique_ptr<mcmc::Learner> learner_ptr;
  try {
    learner_ptr.reset(new mcmc::Learner(cfg, queue));
  } catch (const std::exception& e) {  // the reference LOG(FATAL)s on an unusable configuration (phi.cc:660, learner.cc:146)
    Fatal(e.what());
  }
  mcmc::Learner& learner = *learner_ptr;
  if (!ckptIn.empty()) {
    std::ifstream in(ckptIn, std::ios::binary);
    if (!in.good() || !learner.Parse(&in)) Fatal("cannot restore checkpoint " + ckptIn);
  }
  // with an exchange every rank computes every value (the calls are collectives); the lines carry the rank
  const std::string tag = cfg.exchange ? "I [" + std::to_string(rank) + "] " : "I ";
  std::cerr << tag << "ppx[0] = " << learner.HeldoutPerplexity() << std::endl;
  for (uint64_t i = 0; i < max_iters && !signaled; i += cfg.ppx_interval) {  // main.cc:162-168
    const uint64_t step = std::min<uint64_t>(max_iters - i, cfg.ppx_interval);
    learner.Run(static_cast<uint32_t>(step), &signaled);
    if (!signaled) std::cerr << tag << "ppx[" << i + step << "] = " << learner.HeldoutPerplexity() << std::endl;
    if (!signaled && cfg.calc_train_ppx)
      std::cerr << tag << "train ppx[" << i + step << "] = " << learner.TrainingPerplexity() << std::endl;
  }
  if (signaled) std::cerr << "I FORCED TERMINATE" << std::endl;
  if (!ckptOut.empty()) {
    // Serialize is a collective with an exchange; the states are identical afterwards and rank 0's file is the checkpoint
    std::ofstream out(rank == 0 ? ckptOut : std::string("/dev/null"), std::ios::binary);
    if (!learner.Serialize(&out)) Fatal("cannot write checkpoint " + ckptOut);
  }
  if (!communitiesOut.empty()) {
    // every rank holds all of pi: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(communitiesOut);
        if (!out.good() || !learner.WriteCommunities(&out, static_cast<uint32_t>(membershipTop),
                                                     static_cast<mcmc::Float>(membershipThreshold)))
          Fatal("cannot write communities " + communitiesOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("communities: ") + e.what());
    }
  }
  if (!linksOut.empty()) {
    // every rank holds all of pi: link prediction is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        if (linksNodes.empty()) {
          linkNodes.resize(cfg.N);
          for (uint64_t v = 0; v < cfg.N; ++v) linkNodes[v] = static_cast<mcmc::Vertex>(v);
        }
        std::ofstream out(linksOut);
        if (!out.good() || !learner.WritePredictedLinks(&out, linkNodes, static_cast<uint32_t>(linksTop), linksMask))
          Fatal("cannot write links " + linksOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("links: ") + e.what());
    }
  }
  if (!linkCommOut.empty()) {
    // every rank holds all of pi: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(linkCommOut);
        if (!out.good() || !learner.WriteLinkCommunities(&out, static_cast<uint32_t>(linkCommTop),
                                                         static_cast<mcmc::Float>(linkCommMinTerm)))
          Fatal("cannot write link communities " + linkCommOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("link communities: ") + e.what());
    }
  }
  if (!qualityOut.empty()) {
    // every rank holds all of pi: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(qualityOut);
        if (!out.good() || !learner.WriteCommunityQuality(&out, static_cast<mcmc::Float>(qualityThreshold)))
          Fatal("cannot write community quality " + qualityOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("community quality: ") + e.what());
    }
  }
  if (!coverMatchOut.empty()) {
    // every rank holds all of pi: the comparison is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(coverMatchOut);
        if (!out.good() || !learner.WriteCoverMatch(&out, truthOffsets, truthMembers, static_cast<mcmc::Float>(coverThreshold)))
          Fatal("cannot write cover match " + coverMatchOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("cover match: ") + e.what());
    }
  }
  if (!coverNmiOut.empty()) {
    // every rank holds all of pi: the comparison is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(coverNmiOut);
        if (!out.good() || !learner.WriteCoverNMI(&out, truthOffsets, truthMembers, static_cast<mcmc::Float>(coverThreshold)))
          Fatal("cannot write cover NMI " + coverNmiOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("cover NMI: ") + e.what());
    }
  }
  if (!coverOmegaOut.empty()) {
    // every rank holds all of pi: the comparison is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        const std::vector<uint32_t> universe = mcmc::Learner::OmegaUniverse(
            coverOmegaUniverse.empty() ? "covered" : coverOmegaUniverse, truthMembers, cfg.N);
        std::ofstream out(coverOmegaOut);
        if (!out.good() ||
            !learner.WriteCoverOmega(&out, truthOffsets, truthMembers, static_cast<mcmc::Float>(coverThreshold), universe))
          Fatal("cannot write cover Omega " + coverOmegaOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("cover Omega: ") + e.what());
    }
  }
  if (!relatedOut.empty()) {
    // every rank holds all of pi: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(relatedOut);
        if (!out.good() || !learner.WriteRelatedCommunities(&out, static_cast<mcmc::Float>(relatedThreshold),
                                                            static_cast<uint32_t>(relatedTop),
                                                            relatedBy.empty() ? "jaccard" : relatedBy))
          Fatal("cannot write related communities " + relatedOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("related communities: ") + e.what());
    }
  }
  if (!linkedOut.empty()) {
    // every rank holds all of pi and the training links: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(linkedOut);
        if (!out.good() || !learner.WriteLinkedCommunities(&out, static_cast<mcmc::Float>(linkedThreshold),
                                                           static_cast<uint32_t>(linkedTop),
                                                           linkedBy.empty() ? "density" : linkedBy,
                                                           static_cast<uint64_t>(linkedMinLinks)))
          Fatal("cannot write linked communities " + linkedOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("linked communities: ") + e.what());
    }
  }
  if (!modularityOut.empty()) {
    // every rank holds all of pi and the training links: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(modularityOut);
        if (!out.good() || !learner.WriteModularity(&out, static_cast<mcmc::Float>(modularityThreshold)))
          Fatal("cannot write modularity " + modularityOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("modularity: ") + e.what());
    }
  }
  if (!rolesOut.empty()) {
    // every rank holds all of pi and the training adjacency: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(rolesOut);
        if (!out.good() || !learner.WriteNodeRoles(&out, static_cast<mcmc::Float>(rolesThreshold),
                                                   static_cast<uint32_t>(rolesTop), rolesAmong))
          Fatal("cannot write node roles " + rolesOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("node roles: ") + e.what());
    }
  }
  if (!trianglesOut.empty()) {
    // every rank holds all of pi and the training links: the read-out is local, rank 0's file is the answer
    try {
      if (rank == 0) {
        std::ofstream out(trianglesOut);
        if (!out.good() || !learner.WriteTriangles(&out, static_cast<mcmc::Float>(trianglesThreshold)))
          Fatal("cannot write triangles " + trianglesOut);
      }
    } catch (const std::exception& e) {
      Fatal(std::string("triangles: ") + e.what());
    }
  }
  learner.PrintStats();
  return 0;
}
