// Plan arithmetic of the prefix-sorted 96-bit scan stream (vc_scan_stream.hip builds it, vc_scan_kernel_stream in vc_scan.hip
// reads it): granule headers, the lower bound they give, the layout of the one allocation and the memory rule.  Plain C++ on
// purpose -- no HIP type, no HIP call -- so that the arithmetic also compiles into a stand-alone host program
// (tests/cpp/scan_stream_plan_test.cc).
//
// The stream is a second layout of a 128-bit store, built once per store state: the records sorted by their KEY, which is the
// low 32 bits of code word 0 (bits 0..31 of the code, bytes 0..3 of a record), as four uint32 columns -- key | t0 | t1 | t2 with
// t0 = the high half of word 0, t1 / t2 = the low / high half of word 1 -- plus perm[] (sorted position -> local id) and one
// header per granule of 256 consecutive sorted records.  The verify pass streams t0..t2 only (12 bytes per record); the header
// stands in for the key.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VC_STREAM_HD __host__ __device__
#else
#define VC_STREAM_HD
#endif

#define VC_STREAM_GRANULE 256ull      // sorted records under one header = one wave-load (64 lanes x 4 records)
#define VC_STREAM_CHUNK 2048ull       // records a block takes per step: 8 granules, 6 16-byte loads per lane
#define VC_STREAM_PAD_ITEMS 8192ull   // column stride granularity, as the store's (VC_PAD_ITEMS)
#define VC_STREAM_MEM_SHARE 55u       // per cent of the free device memory a build may take: the share vc_mih_policy gives the
                                      // bucket-order records of an index (vc_mih_policy.hpp)

// the leading key bits that every key of a granule shares (mask, a run of high bits) and their value (prefix, zero elsewhere)
struct VcStreamHeader {
  uint32_t prefix, mask;
};

VC_STREAM_HD static inline uint32_t vc_stream_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// header of a granule whose smallest key is `first` and whose largest is `last` (the keys are sorted, so every key between them
// shares the leading bits the two have in common)
VC_STREAM_HD static inline VcStreamHeader vc_stream_header(uint32_t first, uint32_t last) {
  const uint32_t x = first ^ last;
  const uint32_t common = x ? (uint32_t)__builtin_clz(x) : 32u;
  const uint32_t mask = common ? (0xFFFFFFFFu << (32u - common)) : 0u;
  return VcStreamHeader{first & mask, mask};
}

// least Hamming distance between qkey and any key with the header's prefix: the known bits that differ
VC_STREAM_HD static inline uint32_t vc_stream_key_bound(VcStreamHeader h, uint32_t qkey) { return vc_stream_popc((qkey ^ h.prefix) & h.mask); }

// Start value of an item's accumulate chain in "matching bits" form: the chain adds the matching bits of the 96 streamed bits,
// so chain = tau + (most key bits that can match) + (matching streamed bits) >= tau + 128 - dist, and dist <= tau implies
// chain >= 128.  Unknown key bits count as matching.
VC_STREAM_HD static inline uint32_t vc_stream_chain_start(VcStreamHeader h, uint32_t qkey, uint32_t tau) {
  return tau + (32u - vc_stream_popc(h.mask)) + vc_stream_popc(~(qkey ^ h.prefix) & h.mask);
}

// The kernel splits that formula so that tau never has to become a scalar: the chain starts at the header's part alone, the
// most key bits that can match (wave-uniform, scalar arithmetic) ...
VC_STREAM_HD static inline uint32_t vc_stream_chain_base(VcStreamHeader h, uint32_t qkey) {
  return (32u - vc_stream_popc(h.mask)) + vc_stream_popc(~(qkey ^ h.prefix) & h.mask);
}
// ... and is compared against the fire level of tau: chain_base + matching >= fire_level(tau) <=> chain_start + matching >= 128
// for every tau <= 128 (a larger tau accepts everything, as 128 does).
VC_STREAM_HD static inline uint32_t vc_stream_fire_level(uint32_t tau) { return 128u - (tau < 128u ? tau : 128u); }

// One allocation of uint32 words: key | t0 | t1 | t2 (stride words each) | perm (n_pad) | headers (2 words per granule).
struct VcStreamPlan {
  uint64_t n, n_pad, chunks, granules, stride;
  uint64_t key, t0, perm, hdr;     // word offsets (t1 = t0 + stride, t2 = t0 + 2 * stride)
  uint64_t words, bytes;           // what the engine holds while the stream lives
  uint64_t temp_bytes;             // sort temporaries, freed after the build: the second key / id buffer pair and the sort's work words
};

static inline VcStreamPlan vc_stream_plan(uint64_t n, uint64_t sort_work_words) {
  VcStreamPlan p{};
  p.n = n;
  p.chunks = (n + VC_STREAM_CHUNK - 1) / VC_STREAM_CHUNK;
  p.n_pad = p.chunks * VC_STREAM_CHUNK;
  p.granules = p.n_pad / VC_STREAM_GRANULE;
  p.stride = (p.n_pad + VC_STREAM_PAD_ITEMS - 1) / VC_STREAM_PAD_ITEMS * VC_STREAM_PAD_ITEMS;
  p.key = 0;
  p.t0 = p.stride;
  p.perm = 4 * p.stride;
  p.hdr = p.perm + p.n_pad;
  p.words = p.hdr + 2 * p.granules;
  p.bytes = p.words * 4;
  p.temp_bytes = (2 * n + sort_work_words) * 4;
  return p;
}

// the memory rule: the stream and its build temporaries together within VC_STREAM_MEM_SHARE per cent of the free memory.
// have_free == false (the free-memory query failed): nothing is known, the allocation itself decides.
static inline bool vc_stream_fits(const VcStreamPlan& p, bool have_free, uint64_t free_bytes) {
  return !have_free || p.bytes + p.temp_bytes <= free_bytes / 100 * VC_STREAM_MEM_SHARE;
}

// bytes one verify launch over the stream reads: the three hot columns of every padded record and every granule header
static inline uint64_t vc_stream_scan_bytes(const VcStreamPlan& p) { return p.n_pad * 12 + p.granules * 8; }
