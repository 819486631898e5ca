// Test helper: the ingest loop of a running store through the drop-in layer -- vc::GpuProxy::put(ID, BinaryCode) per record as a
// loader does, vc::Backend::update_index() instead of a rebuild, get(HashIndex, Image_List) as search_worker.cc:246 asks.
// 64-bit codes, 4 tables: table 0's key is the first two code bytes.  Prints the ids of bucket (0, 0x1234).
#include <stdio.h>

#include "verticut_host.hpp"

using namespace vc;

int main() {
  const uint32_t n0 = 40, extra = 5;
  Engine eng(64, 4, n0 + extra);
  GpuProxy proxy(&eng);
  auto put = [&](uint32_t id, uint16_t key0) {
    ID k; k.set_id(id);
    unsigned char c[8] = {(unsigned char)(key0 & 255), (unsigned char)(key0 >> 8), (unsigned char)id, 1, 2, 3, 4, 5};
    BinaryCode v; v.set_code((const char*)c, 8);
    return proxy.put(k, v);
  };
  for (uint32_t i = 0; i < n0; ++i) if (put(i, i % 4 == 0 ? 0x1234 : (uint16_t)(0x2000 + i)) != PROXY_PUT_DONE) return 10;
  if (eng.build_index() != VC_OK) return 11;
  for (uint32_t i = n0; i < n0 + extra; ++i) if (put(i, i == n0 + 2 ? 0x1234 : (uint16_t)(0x4000 + i)) != PROXY_PUT_DONE) return 12;
  HashIndex hi; hi.set_table_id(0); hi.set_index(0x1234);
  Image_List got;
  bool stale_refused = false;
  try { proxy.get(hi, got); } catch (const EngineError& e) { stale_refused = e.code() == VC_ERR_STATE; }
  if (!stale_refused) return 13;
  Backend* b = &eng;
  if (b->update_index() != VC_OK) return 14;
  if (proxy.get(hi, got) != PROXY_FOUND) return 15;
  printf("bucket");
  for (int i = 0; i < got.images_size(); ++i) printf(" %u", got.images(i).id());
  printf("\n");
  HashIndex fresh; fresh.set_table_id(0); fresh.set_index(0x4000 + n0);
  if (proxy.get(fresh, got) != PROXY_FOUND || got.images_size() != 1 || got.images(0).id() != n0) return 16;
  return 0;
}
