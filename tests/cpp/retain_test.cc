// Test helper: records taken out of a running store through the drop-in layer -- vc::Backend::retain on both backends (one engine,
// three shards on one device), then get(HashIndex, Image_List) as search_worker.cc:246 asks and get(ID, BinaryCode).
// 64-bit codes, 4 tables: table 0's key is the first two code bytes, byte 2 carries the record's ORIGINAL id.  Every third record is
// removed; bucket (0, 0x1234) held the records 0, 4, 8, ...  Prints, per backend, n_kept and the bucket's new ids.
#include <stdio.h>

#include <vector>

#include "verticut_host.hpp"

using namespace vc;

static int run(Backend* b, const char* name) {
  const uint32_t n = 40;
  GpuProxy proxy(b);
  for (uint32_t i = 0; i < n; ++i) {
    const uint16_t key0 = i % 4 == 0 ? 0x1234 : (uint16_t)(0x2000 + i);
    ID k; k.set_id(i);
    unsigned char c[8] = {(unsigned char)(key0 & 255), (unsigned char)(key0 >> 8), (unsigned char)i, 1, 2, 3, 4, 5};
    BinaryCode v; v.set_code((const char*)c, 8);
    if (proxy.put(k, v) != PROXY_PUT_DONE) return 10;
  }
  if (b->build_index() != VC_OK) return 11;
  std::vector<uint32_t> sel(n), map(n, 7u);
  for (uint32_t i = 0; i < n; ++i) sel[i] = i % 3 != 0;
  uint64_t kept = 0;
  if (b->retain(sel.data(), VC_RETAIN_MASK, map.data(), &kept) != VC_OK) return 12;
  if (kept != b->size()) return 13;
  uint32_t next = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (map[i] != (sel[i] ? next++ : 0xFFFFFFFFu)) return 14;
  HashIndex hi; hi.set_table_id(0); hi.set_index(0x1234);
  Image_List got;
  if (proxy.get(hi, got) != PROXY_FOUND) return 15;
  printf("%s kept %llu bucket", name, (unsigned long long)kept);
  for (int i = 0; i < got.images_size(); ++i) {
    printf(" %u", got.images(i).id());
    if ((unsigned char)got.images(i).code()[2] % 4 != 0) return 16;                 // the record that moved here is a bucket member
    if (map[(unsigned char)got.images(i).code()[2]] != got.images(i).id()) return 17;   // ... at the id the map names
  }
  printf("\n");
  HashIndex gone; gone.set_table_id(0); gone.set_index(0x2000 + 3);                  // record 3 was alone in its bucket
  if (proxy.get(gone, got) == PROXY_FOUND) return 18;
  if (b->retain(nullptr, VC_RETAIN_MASK, nullptr, nullptr) != VC_ERR_INVALID || b->retain(sel.data(), 2, nullptr, nullptr) != VC_ERR_INVALID) return 19;
  return 0;
}

int main() {
  {
    Engine eng(64, 4, 45);
    if (int rc = run(&eng, "engine")) return rc;
  }
  {
    ShardedEngine sh(64, 4, 50, 3, {0});
    if (int rc = run(&sh, "sharded")) return 100 + rc;
  }
  return 0;
}
