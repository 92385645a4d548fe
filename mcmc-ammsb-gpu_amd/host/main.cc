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

// A flag that modifies one post-fit output (new, as are all of them).  It knows whether it was given -- it then needs
// its output's flag -- reads the whole of its argument ("4x" is invalid), and carries its own range rule.
struct Modifier {
  std::string name, help;
  bool given = false;
  Modifier(const std::string& n, const std::string& h) : name(n), help(h) {}
  virtual ~Modifier() {}
  virtual bool Set(const std::string& v) = 0;
  virtual std::string MustBe() const = 0;  // the value's rule where the value breaks it ("in 1..16"), else ""
  void Check() const {
    const std::string rule = MustBe();
    if (!rule.empty()) Fatal("--" + name + " must be " + rule);
  }
  Option AsOption() {
    return Option{name, 0, help, [this](const std::string& v) {
                    given = true;
                    return Set(v);
                  }};
  }

 protected:
  template <class T>
  static bool Parse(const std::string& v, T* x) {
    std::istringstream in(v);
    in >> *x;
    return !in.fail() && in.eof();
  }
};

// pi[a, k] >= value makes a a member of k.  The libraries take a binary32, so that is what has to be finite;
// --membership-threshold alone (finite = false) keeps its older rule.
struct Threshold : Modifier {
  double value;
  bool finite;
  Threshold(const std::string& n, double def, const std::string& h, bool f = true) : Modifier(n, h), value(def), finite(f) {}
  bool Set(const std::string& v) override { return Parse(v, &value); }
  std::string MustBe() const override {
    if (value >= 0 && (!finite || std::isfinite(static_cast<float>(value)))) return "";
    return finite ? "finite and >= 0" : ">= 0";
  }
};

// how many entries a row of the output keeps at the most
struct Top : Modifier {
  long value, max;
  Top(const std::string& n, long def, long mx, const std::string& h) : Modifier(n, h), value(def), max(mx) {}
  bool Set(const std::string& v) override { return Parse(v, &value); }
  std::string MustBe() const override { return value < 1 || value > max ? "in 1.." + std::to_string(max) : ""; }
};

struct Count : Modifier {
  long long value;
  Count(const std::string& n, long long def, const std::string& h) : Modifier(n, h), value(def) {}
  bool Set(const std::string& v) override { return Parse(v, &value); }
  std::string MustBe() const override { return value < 0 ? ">= 0" : ""; }
};

// One of a few words.  The choices that --help shows no default for take an empty argument as not given.
struct Choice : Modifier {
  std::vector<std::string> words;
  std::string def, value;
  bool emptyIsDefault;
  Choice(const std::string& n, const std::vector<std::string>& w, const std::string& d, const std::string& h = "")
      : Modifier(n, h), words(w), def(d), emptyIsDefault(h.empty()) {}
  bool Set(const std::string& v) override {
    value = v;
    given = !(emptyIsDefault && v.empty());
    return true;
  }
  const std::string& Get() const { return given ? value : def; }
  std::string MustBe() const override {
    if (std::find(words.begin(), words.end(), Get()) != words.end()) return "";
    std::string list;
    for (size_t i = 0; i < words.size(); ++i) list += (i == 0 ? "" : i + 1 == words.size() ? " or " : ", ") + words[i];
    return list;
  }
};

struct Text : Modifier {
  std::string value;
  explicit Text(const std::string& n) : Modifier(n, "") {}
  bool Set(const std::string& v) override {
    value = v;
    given = !v.empty();
    return true;
  }
  std::string MustBe() const override { return ""; }
};

// One post-fit output: --FLAG FILE makes rank 0 write FILE after the last perplexity line.
struct Output {
  std::string flag;
  std::string words;                 // "cannot write WORDS FILE", "WORDS: what the writer threw"
  std::vector<Modifier*> modifiers;  // each of them needs --FLAG
  std::function<bool(mcmc::Learner&, std::ostream*)> write;
  std::string file = "";
};

}  // namespace

int main(int argc, char** argv) {
  {
    std::ostringstream s;
    for (int i = 0; i < argc; ++i) s << argv[i] << " ";
    std::cerr << "I " << s.str() << std::endl;
  }
  std::string filename, loadFile, dumpFile, ckptIn, ckptOut, exchangeKind, groundTruth;
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
  };

  // The post-fit outputs (all new): each one's modifiers, then its entry in the table below.
  Top membershipTop("membership-top", 4, 16, "4 (new, with --communities-out: strongest communities kept per node, 1..16)");
  Threshold membershipThreshold("membership-threshold", 0, "0 (new, with --communities-out: a node is a member where pi >= this)", false);
  Top linksTop("links-top", 10, 64, "10 (new, with --links-out: most probable partners kept per node, 1..64)");
  Text linksNodes("links-nodes");  // file of query node ids; default: every node
  Choice linksExclude("links-exclude", {"none", "training", "all"}, "all");  // all = training and held-out edges
  Top linkCommTop("link-communities-top", 1, 16, "1 (new, with --link-communities-out: largest terms kept per link, 1..16)");
  Threshold linkCommMinTerm("link-communities-min-term", 0, "0 (new, with --link-communities-out: terms below it take no slot)");
  Threshold qualityThreshold("community-quality-threshold", 0.05, "0.05 (new, with --community-quality-out: a node is a member of k iff pi[a, k] >= it)");
  // the three cover outputs share this threshold; its rules are written out below
  Threshold coverThreshold("cover-match-threshold", 0.05, "0.05 (new, with --ground-truth and --cover-match-out: a node is a member of k iff pi[a, k] >= it)");
  Choice coverOmegaUniverse("cover-omega-universe", {"covered", "all"}, "covered");  // covered = the nodes some ground-truth community holds
  Threshold relatedThreshold("related-communities-threshold", 0.05, "0.05 (new, with --related-communities-out: a node is a member of k iff pi[a, k] >= it)");
  Top relatedTop("related-communities-top", 4, 64, "4 (new, with --related-communities-out: closest communities kept per community, 1..64)");
  Choice relatedBy("related-communities-by", {"jaccard", "overlap", "contained"}, "jaccard");
  Threshold linkedThreshold("linked-communities-threshold", 0.05, "0.05 (new, with --linked-communities-out: a node is a member of k iff pi[a, k] >= it)");
  Top linkedTop("linked-communities-top", 4, 64, "4 (new, with --linked-communities-out: partners kept per community, 1..64)");
  Choice linkedBy("linked-communities-by", {"density", "links"}, "density");
  Count linkedMinLinks("linked-communities-min-links", 1, "1 (new, with --linked-communities-out: fewest links that make a partner)");
  Threshold modularityThreshold("modularity-threshold", 0.05, "0.05 (new, with --modularity-out: a node is a member of k iff pi[a, k] >= it)");
  Threshold rolesThreshold("node-roles-threshold", 0.05, "0.05 (new, with --node-roles-out: a node is a member of k iff pi[a, k] >= it)");
  Top rolesTop("node-roles-top", 4, 16, "4 (new, with --node-roles-out: communities kept per node, 1..16)");
  Choice rolesAmong("node-roles-among", {"all", "own"}, "all", "all (new, with --node-roles-out: all = every community a neighbour is in, own = the node's own)");
  Threshold trianglesThreshold("triangles-threshold", 0.05, "0.05 (new, with --triangles-out: a node is a member of k iff pi[a, k] >= it)");

  using mcmc::Float;
  using mcmc::Learner;
  std::vector<uint64_t> truthOffsets;  // --ground-truth, a SNAP cmty file: one community per line; the graph file's own
  std::vector<uint32_t> truthMembers;  // ids with --file, dense ids with --load-data
  std::vector<mcmc::Vertex> linkNodes;
  // In the order the files are written.  Every rank holds all of pi and the training graph, so each analysis is local and
  // rank 0's file is the answer.  Each file starts with a `#` line, quoted here with the lines that follow it.
  Output outputs[] = {
      // `# N K top threshold`, then `k size n0 n1 ...` per community
      {"communities-out", "communities", {&membershipTop, &membershipThreshold},
       [&](Learner& l, std::ostream* out) {
         return l.WriteCommunities(out, static_cast<uint32_t>(membershipTop.value), static_cast<Float>(membershipThreshold.value));
       }},
      // `# N K top exclude`, then `a n b0 s0 b1 s1 ...` per query node
      {"links-out", "links", {&linksTop, &linksNodes, &linksExclude},
       [&](Learner& l, std::ostream* out) {
         if (!linksNodes.given) {
           linkNodes.resize(cfg.N);
           for (uint64_t v = 0; v < cfg.N; ++v) linkNodes[v] = static_cast<mcmc::Vertex>(v);
         }
         const std::string& exclude = linksExclude.Get();
         const uint32_t mask = exclude == "none" ? 0 : exclude == "training" ? Learner::kExcludeTraining
                                                                             : Learner::kExcludeTraining | Learner::kExcludeHeldout;
         return l.WritePredictedLinks(out, linkNodes, static_cast<uint32_t>(linksTop.value), mask);
       }},
      // `# N K E top min_term`, then `a b p n k0 t0 k1 t1 ...` per training link
      {"link-communities-out", "link communities", {&linkCommTop, &linkCommMinTerm},
       [&](Learner& l, std::ostream* out) {
         return l.WriteLinkCommunities(out, static_cast<uint32_t>(linkCommTop.value), static_cast<Float>(linkCommMinTerm.value));
       }},
      // `# N K E threshold uncovered`, then `k size internal boundary conductance density` per community
      {"community-quality-out", "community quality", {&qualityThreshold},
       [&](Learner& l, std::ostream* out) { return l.WriteCommunityQuality(out, static_cast<Float>(qualityThreshold.value)); }},
      // (with --ground-truth) `# N K G threshold skipped f1_truth f1_detected avg_f1`, then `t g size best overlap f1` per
      // ground-truth and `d k size best overlap f1` per detected community
      {"cover-match-out", "cover match", {},
       [&](Learner& l, std::ostream* out) {
         return l.WriteCoverMatch(out, truthOffsets, truthMembers, static_cast<Float>(coverThreshold.value));
       }},
      // (with --ground-truth) `# N K G threshold skipped nmi_lfk nmi_max`, then `t g size H h` per ground-truth and
      // `d k size H h` per detected community (H the entropy, h the conditional entropy given the other cover; %.17g)
      {"cover-nmi-out", "cover NMI", {},
       [&](Learner& l, std::ostream* out) {
         return l.WriteCoverNMI(out, truthOffsets, truthMembers, static_cast<Float>(coverThreshold.value));
       }},
      // (with --ground-truth) `# N K G threshold universe_n skipped outside omega omega_unadjusted`, then
      // `j agree detected truth` per level: the pairs of the universe that share j communities (%.17g, `nan` where undefined)
      {"cover-omega-out", "cover Omega", {&coverOmegaUniverse},
       [&](Learner& l, std::ostream* out) {
         const std::vector<uint32_t> universe = Learner::OmegaUniverse(coverOmegaUniverse.Get(), truthMembers, cfg.N);
         return l.WriteCoverOmega(out, truthOffsets, truthMembers, static_cast<Float>(coverThreshold.value), universe);
       }},
      // `# N K threshold by top min_overlap`, then `k size n l0 o0 l1 o1 ...` per community: its n closest other
      // communities and the nodes it shares with each
      {"related-communities-out", "related communities", {&relatedThreshold, &relatedTop, &relatedBy},
       [&](Learner& l, std::ostream* out) {
         return l.WriteRelatedCommunities(out, static_cast<Float>(relatedThreshold.value), static_cast<uint32_t>(relatedTop.value),
                                          relatedBy.Get());
       }},
      // `# N K E threshold by top min_links skipped`, then `k size internal n l0 w0 o0 l1 w1 o1 ...` per community: the n
      // other communities it is linked to most, the training links to each and the nodes shared with each
      {"linked-communities-out", "linked communities", {&linkedThreshold, &linkedTop, &linkedBy, &linkedMinLinks},
       [&](Learner& l, std::ostream* out) {
         return l.WriteLinkedCommunities(out, static_cast<Float>(linkedThreshold.value), static_cast<uint32_t>(linkedTop.value),
                                         linkedBy.Get(), static_cast<uint64_t>(linkedMinLinks.value));
       }},
      // `# N K E threshold skipped q`, then `k q_k in_k s_k internal volume` per community: the overlapping modularity of
      // the cover against the training links, the 128-bit sums as 32 hexadecimal digits
      {"modularity-out", "modularity", {&modularityThreshold},
       [&](Learner& l, std::ostream* out) { return l.WriteModularity(out, static_cast<Float>(modularityThreshold.value)); }},
      // `# N K M threshold among top min_count skipped`, `c k members ksum ksq` per community,
      // `n a degree own embedded reached votes squares nslots k0 c0 f0 ...` per node: how each node sits in the cover
      // against the training adjacency
      {"node-roles-out", "node roles", {&rolesThreshold, &rolesTop, &rolesAmong},
       [&](Learner& l, std::ostream* out) {
         return l.WriteNodeRoles(out, static_cast<Float>(rolesThreshold.value), static_cast<uint32_t>(rolesTop.value), rolesAmong.Get());
       }},
      // `# N K M threshold skipped dropped total`, `c k members part tri3 wedges` per community,
      // `n a degree tri tri_in tri_comms` per node: the triangles of the training adjacency inside the detected communities
      {"triangles-out", "triangles", {&trianglesThreshold},
       [&](Learner& l, std::ostream* out) { return l.WriteTriangles(out, static_cast<Float>(trianglesThreshold.value)); }},
  };
  auto output = [&](const std::string& flag) -> Output& {
    for (Output& o : outputs)
      if (o.flag == flag) return o;
    Fatal("the table of outputs has no --" + flag);
  };
  Output &communities = output("communities-out"), &links = output("links-out"), &coverMatch = output("cover-match-out"),
         &coverNmi = output("cover-nmi-out"), &coverOmega = output("cover-omega-out");
  // --help lists each output's flag and then its modifiers, in the table's order but for the two oldest: --links-out
  // comes after the rest, and --communities-out's modifiers last of all
  auto flag = [&](Output& o) { options.push_back(OptStr(o.flag, 0, &o.file)); };
  auto modifiers = [&](Output& o) {
    for (Modifier* m : o.modifiers) options.push_back(m->AsOption());
  };
  flag(communities);
  for (Output& o : outputs) {
    if (&o == &communities || &o == &links) continue;
    if (&o == &coverMatch) options.push_back(OptStr("ground-truth", 0, &groundTruth));
    flag(o);
    modifiers(o);
    if (&o == &coverOmega) options.push_back(coverThreshold.AsOption());
  }
  flag(links);
  modifiers(links);
  modifiers(communities);
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
  for (const Output& o : outputs) {
    std::string names;
    bool given = false;
    for (const Modifier* m : o.modifiers) {
      names += (names.empty() ? "--" : " / --") + m->name;
      given = given || m->given;
    }
    if (given && o.file.empty()) Fatal(names + (o.modifiers.size() == 1 ? " needs --" : " need --") + o.flag + " FILE");
    for (const Modifier* m : o.modifiers) m->Check();
  }
  // the cover outputs need --ground-truth, it needs one of them, and so does the threshold they share
  const bool noCoverOut = coverMatch.file.empty() && coverNmi.file.empty() && coverOmega.file.empty();
  if (groundTruth.empty() && !coverMatch.file.empty()) Fatal("--ground-truth FILE and --cover-match-out FILE need each other");
  if (groundTruth.empty() && !coverNmi.file.empty()) Fatal("--cover-nmi-out FILE needs --ground-truth FILE");
  if (groundTruth.empty() && !coverOmega.file.empty()) Fatal("--cover-omega-out FILE needs --ground-truth FILE");
  if (!groundTruth.empty() && noCoverOut)
    Fatal("--ground-truth FILE and --cover-match-out FILE need each other (or --cover-nmi-out FILE, or --cover-omega-out FILE)");
  if (coverThreshold.given && noCoverOut)
    Fatal("--cover-match-threshold needs --ground-truth FILE and --cover-match-out FILE (or --cover-nmi-out FILE, or --cover-omega-out FILE)");
  coverThreshold.Check();
  if (linksNodes.given) {
    std::ifstream in(linksNodes.value);
    if (!in.good()) Fatal("cannot read --links-nodes file " + linksNodes.value);
    unsigned long long v;
    while (in >> v) {
      if (v > 0xFFFFFFFFull) Fatal("--links-nodes: node id " + std::to_string(v) + " is not a node id");
      linkNodes.push_back(static_cast<mcmc::Vertex>(v));
    }
    if (!in.eof()) Fatal("--links-nodes: " + linksNodes.value + " holds something that is not a node id");
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
  for (Output& o : outputs) {
    if (o.file.empty()) continue;
    try {
      if (rank == 0) {
        std::ofstream out(o.file);
        if (!out.good() || !o.write(learner, &out)) Fatal("cannot write " + o.words + " " + o.file);
      }
    } catch (const std::exception& e) {
      Fatal(o.words + ": " + e.what());
    }
  }
  learner.PrintStats();
  return 0;
}
