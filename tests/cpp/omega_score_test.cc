// mcmc::Learner::OmegaIndex::Derive without a device: reads lines `n a0,a1,.. d0,d1,.. t0,t1,..` (the universe's size
// and the three histograms, unsigned 64-bit) from standard input and prints `omega omega_unadjusted` per line, %.17g,
// NaN as `nan`.  tests/test_omega_host.py compares the output with fractions.Fraction rounded once.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mcmc/learner.h"

static std::vector<uint64_t> Parse(const std::string& list) {
  std::vector<uint64_t> v;
  std::stringstream ss(list);
  std::string item;
  while (std::getline(ss, item, ',')) v.push_back(strtoull(item.c_str(), nullptr, 10));
  return v;
}

static void Print(double x, const char* end) {
  if (x != x) printf("nan%s", end);
  else printf("%.17g%s", x, end);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::stringstream ss(line);
    std::string n, a, d, t;
    if (!(ss >> n >> a >> d >> t)) continue;
    mcmc::Learner::OmegaIndex r;
    r.nodes = strtoull(n.c_str(), nullptr, 10);
    r.agree = Parse(a);
    r.detected = Parse(d);
    r.truth = Parse(t);
    if (r.agree.size() != r.detected.size() || r.agree.size() != r.truth.size()) return 2;
    r.Derive();
    Print(r.omega, " ");
    Print(r.omega_unadjusted, "\n");
  }
  return 0;
}
