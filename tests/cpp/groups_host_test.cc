// Test helper: vc::Backend::group_summary on both backends (one engine, three shards on one device) through the drop-in layer, then
// retain() of rep_labels with VC_RETAIN_ROOTS.  48 records of 64 bits, code byte j of record i = (i * 37 + j * 11 + (i % 5) * j) & 255,
// label of record i = (i * 7) % 9 -- tests/test_groups_gpu.py builds the same and compares the printed line with the numpy model.
// Prints per backend: name, G, then per group "label:size:rep:rep_dist:max_dist:centroid-hex", then the rep_labels, then n_kept.
#include <stdio.h>

#include <vector>

#include "verticut_host.hpp"

using namespace vc;

static int run(Backend* b, const char* name) {
  const uint32_t n = 48;
  std::vector<unsigned char> codes(n * 8);
  std::vector<uint32_t> labels(n), rep_labels(n, 7u), group_index(n, 7u);
  for (uint32_t i = 0; i < n; ++i) {
    for (uint32_t j = 0; j < 8; ++j) codes[i * 8 + j] = (unsigned char)((i * 37 + j * 11 + (i % 5) * j) & 255);
    labels[i] = (i * 7) % 9;
  }
  if (b->add_codes(codes.data(), n) != VC_OK) return 10;
  std::vector<vc_group> groups(n);
  std::vector<unsigned char> cents(n * 8);
  uint64_t G = 99;
  if (b->group_summary(labels.data(), 3, groups.data(), cents.data(), nullptr, nullptr, &G) != VC_ERR_CAPACITY || G != 9) return 11;
  if (b->group_summary(labels.data(), n, groups.data(), cents.data(), rep_labels.data(), group_index.data(), &G) != VC_OK) return 12;
  printf("%s %llu", name, (unsigned long long)G);
  for (uint64_t g = 0; g < G; ++g) {
    printf(" %u:%u:%u:%u:%u:", groups[g].label, groups[g].size, groups[g].rep, groups[g].rep_dist, groups[g].max_dist);
    for (int j = 0; j < 8; ++j) printf("%02x", cents[g * 8 + j]);
    if (groups[g].reserved != 0) return 13;
  }
  printf(" |");
  for (uint32_t i = 0; i < n; ++i) {
    printf(" %u", rep_labels[i]);
    if (groups[group_index[i]].label != labels[i]) return 14;
  }
  uint64_t kept = 0;
  if (b->retain(rep_labels.data(), VC_RETAIN_ROOTS, nullptr, &kept) != VC_OK) return 15;
  printf(" | %llu\n", (unsigned long long)kept);
  labels[5] = (uint32_t)b->size();   // one past the resident range
  const int rc = b->group_summary(labels.data(), n, groups.data(), nullptr, nullptr, nullptr, &G);
  if (rc != VC_ERR_INVALID) {
    fprintf(stderr, "%s: a label one past the range gave %d (%s)\n", name, rc, b->last_error());
    return 16;
  }
  if (b->group_summary(nullptr, n, groups.data(), nullptr, nullptr, nullptr, &G) != VC_ERR_INVALID) return 17;
  return 0;
}

int main() {
  {
    Engine eng(64, 4, 60);
    if (int rc = run(&eng, "engine")) return rc;
  }
  {
    ShardedEngine sh(64, 4, 60, 3, {0});
    if (int rc = run(&sh, "sharded")) return 100 + rc;
  }
  return 0;
}
