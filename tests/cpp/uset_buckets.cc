// Test helper (built on the fly by tests/test_refsample_host.py): bucket_count() of a REAL std::unordered_set after each
// unique insert, to pin the epoch table libammsb_refsample.so records at creation.
#include <cstdint>
#include <unordered_set>
extern "C" uint64_t real_uset_bucket_history(const uint64_t* keys, uint64_t n, uint64_t* buckets_after) {
  std::unordered_set<uint64_t> s;
  uint64_t c = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (s.insert(keys[i]).second) buckets_after[c++] = s.bucket_count();
  return c;
}
