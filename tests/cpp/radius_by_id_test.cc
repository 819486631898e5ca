// Test helper: vc::image_search_client::search_image_by_id_within through the drop-in layer on one engine.
// usage: radius_by_id_test <code file> <n> <bits> <tables> <radius> <id_flags> <id>...
// Prints one line per id: "id <id> :" followed by " <image id>:<dist>" pairs in the order the call returns them.
#include <stdio.h>
#include <stdlib.h>

#include "verticut_host.hpp"

using namespace vc;

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const uint64_t n = strtoull(argv[2], nullptr, 10);
  const uint32_t bits = (uint32_t)atoi(argv[3]), m = (uint32_t)atoi(argv[4]), radius = (uint32_t)atoi(argv[5]);
  const uint32_t id_flags = (uint32_t)strtoul(argv[6], nullptr, 0);
  Engine eng(bits, m, n);
  uint64_t n_read = 0;
  if (eng.load_code_file(argv[1], 0, &n_read) != VC_OK || n_read != n) return 10;
  if (eng.build_index() != VC_OK) return 11;
  image_search_client client(&eng);
  for (int a = 7; a < argc; ++a) {
    const uint32_t id = (uint32_t)strtoul(argv[a], nullptr, 10);
    printf("id %u :", id);
    for (const auto& p : id_flags == VC_IDS_EXCLUDE_SELF ? client.search_image_by_id_within(id, radius)   // the default argument
                                                         : client.search_image_by_id_within(id, radius, id_flags))
      printf(" %u:%u", p.first, p.second);
    printf("\n");
  }
  return 0;
}
