// ============================================================================
// verticut_host.hpp -- C++ host layer above the C ABI (include/verticut_gpu.h), shaped like the
// reference's own interfaces for this path so its callers can switch over:
//
//   vc::BaseProxy<K,V>        same virtuals / return codes as src/base_proxy.h:10-29
//   vc::GpuProxy              BaseProxy over the HBM-resident index:
//                               HashIndex{table_id,index} -> Image_List   (search_worker.cc:224-246)
//                               ID{id}                    -> BinaryCode   (linear_search.cc:45-46)
//   vc::SearchWorker          find(code, nbytes, knn, approximate) / get_knn / get_stat
//                             (src/search_worker.h:25-33); results farthest first (search_worker.cc:210-216)
//   vc::image_search_client   ping / search_image_by_id(id, knn, approximate)
//                             (src/image_search_client.h:12-27), in process instead of msgpack-rpc;
//                             search_images_by_id (a batch), search_image_by_id_within (all images within a radius)
//
// The message structs stand in for the protobuf messages of src/image_search.proto:3-27 (same field
// names and accessors; no wire format -- there is no KV tier to talk to any more).
// Header only; needs libverticut_gpu.so at link time.  No CPU search path: every call lands in the C ABI.
// ============================================================================
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <list>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/verticut_gpu.h"

namespace vc {

// ---- src/base_proxy.h:10-13
enum { PROXY_FOUND = 0, PROXY_NOT_FOUND = 1, PROXY_PUT_DONE = 0, PROXY_PUT_FAIL = 1 };

// ---- src/image_search.proto:3-27 (field semantics only)
struct Message { virtual ~Message() {} };
struct ID : Message {
  uint32_t id_ = 0;
  void set_id(uint32_t v) { id_ = v; }
  uint32_t id() const { return id_; }
};
struct BinaryCode : Message {
  std::string code_;
  void set_code(const char* p, size_t n) { code_.assign(p, n); }
  const std::string& code() const { return code_; }
};
struct HashIndex : Message {
  uint32_t table_id_ = 0, index_ = 0;
  void set_table_id(uint32_t v) { table_id_ = v; }
  void set_index(uint32_t v) { index_ = v; }
  uint32_t table_id() const { return table_id_; }
  uint32_t index() const { return index_; }
};
struct ID_Code_Pair : Message {
  uint32_t id_ = 0;
  std::string code_;
  void set_id(uint32_t v) { id_ = v; }
  void set_code(const char* p, size_t n) { code_.assign(p, n); }
  uint32_t id() const { return id_; }
  const std::string& code() const { return code_; }
};
struct Image_List : Message {
  std::vector<ID_Code_Pair> images_;
  int images_size() const { return (int)images_.size(); }
  const ID_Code_Pair& images(int i) const { return images_[i]; }
  ID_Code_Pair* add_images() { images_.emplace_back(); return &images_.back(); }
  void clear_images() { images_.clear(); }
};

// ---- src/base_proxy.h:15-29
template <class K, class V>
class BaseProxy {
 public:
  virtual ~BaseProxy() {}
  virtual int get(const K& key, V& value) = 0;
  virtual int put(const K& key, const V& value) = 0;
  virtual int contain(const K& key) = 0;
  virtual int init(const char* filename) = 0;
  virtual void close() = 0;
};

class EngineError : public std::runtime_error {
 public:
  EngineError(int code, const std::string& what) : std::runtime_error(what), code_(code) {}
  int code() const { return code_; }
 private:
  int code_;
};

// What the adapters below need from the store: one GPU (Engine) or the GPUs of a node (ShardedEngine).
class Backend {
 public:
  virtual ~Backend() {}
  virtual uint32_t bits() const = 0;
  virtual uint32_t n_tables() const = 0;
  uint32_t nbytes() const { return bits() / 8; }
  virtual const char* last_error() const = 0;
  void check(int rc) const {
    if (rc < 0) throw EngineError(rc, last_error());
  }
  virtual int add_codes(const void* codes, uint64_t n) = 0;
  virtual int load_code_file(const char* path, uint64_t max_records, uint64_t* n_read) = 0;
  virtual int build_index() = 0;
  // the records put since the last build / update are appended to their buckets (vc_update_index: build_hash_tables.cc:40-70)
  virtual int update_index() = 0;
  virtual uint64_t size() const = 0;
  virtual int get_code(uint32_t id, void* out) = 0;
  virtual int get_bucket(uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n) = 0;
  virtual int search_knn(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint64_t* out,
                         uint32_t* counts, vc_query_stats* stats) = 0;
  // a batch of queries named by id (vc_search_knn_ids / vc_sharded_search_knn_ids): the codes never leave HBM
  virtual int search_knn_ids(const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint32_t id_flags,
                             uint64_t* out, uint32_t* counts, vc_query_stats* stats) = 0;
  // all items within `radius` of a batch of records named by id (vc_search_radius_ids / vc_sharded_search_radius_ids)
  virtual int search_radius_ids(const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags, uint64_t* out,
                                uint64_t out_cap, uint64_t* out_offsets) = 0;
  // near-duplicate groups: labels[i] = smallest id of the component of record i in the radius graph (vc_cluster_radius /
  // vc_sharded_cluster_radius; labels[0 .. n_labelled) come in for the incremental form)
  virtual int cluster_radius(uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_cluster_stats* stats) = 0;
  // the same at every radius 0 .. max_radius from one walk: labels is level-major, (max_radius + 1) x size(), row r = cluster_radius(r);
  // stats->n_pairs[d] = the pairs at distance exactly d, n_clusters[r] = the groups at radius r (vc_cluster_levels /
  // vc_sharded_cluster_levels; of every row the first n_labelled entries come in for the incremental form)
  virtual int cluster_levels(uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_levels_stats* stats) = 0;
  // greedy leader dedup: labels[i] = own id for a LEADER (no leader with a smaller id within `radius`), else the smallest-id leader
  // within `radius` (vc_leaders_radius / vc_sharded_leaders_radius; labels[0 .. n_labelled) come in, read only); retain() with
  // VC_RETAIN_ROOTS keeps exactly the leaders
  virtual int leaders_radius(uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_leader_stats* stats) = 0;
  // density clustering: degrees[i] (may be null) = records within `radius` of record i, itself included; a CORE has at least min_pts;
  // labels[i] = the smallest core id of a core's component, the label of a border's smallest-id core neighbour, the own id for noise
  // (vc_dbscan_radius / vc_sharded_dbscan_radius); retain() with VC_RETAIN_ROOTS keeps one record per cluster and the noise
  virtual int dbscan_radius(uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* degrees, vc_dbscan_stats* stats) = 0;
  // the same at every radius 0 .. max_radius from one walk: labels is level-major, (max_radius + 1) x size(), row r = dbscan_radius(r,
  // min_pts); core_dist[i] (may be null) = the distance to record i's min_pts-th nearest record, itself counted, VC_CORE_NEVER for
  // none within max_radius -- a core at level r iff core_dist[i] <= r (vc_dbscan_levels / vc_sharded_dbscan_levels)
  virtual int dbscan_levels(uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* core_dist, vc_dbscan_levels_stats* stats) = 0;
  // the groups of equal labels summarised (vc_group_summary / vc_sharded_group_summary): sizes, per-bit majority codes, the member
  // nearest each -- retain() of rep_labels with VC_RETAIN_ROOTS keeps exactly these representatives
  virtual int group_summary(const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels, uint32_t* group_index,
                            uint64_t* n_groups) = 0;
  // the nearest of n_centres given codes for the records first .. first + count - 1 (vc_assign_nearest / vc_sharded_assign_nearest):
  // out[j] = centre index | distance << 32, a tie in distance goes to the smaller index
  virtual int assign_nearest(const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out) = 0;
  // k-majority over all records (vc_kmajority / vc_sharded_kmajority): centres in as seeds, out as the final centres; assign as
  // assign_nearest(centres) over everything; labels (may be null) = id_base + centre index, a legal input of group_summary()
  virtual int kmajority(uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels, vc_kmajority_stats* stats) = 0;
  // seeds for kmajority() made on the device (vc_seed_centres / vc_sharded_seed_centres): method VC_SEED_FARTHEST or VC_SEED_WEIGHTED;
  // centres out; picks (id | pick distance << 32), assign (as assign_nearest(centres) over everything) and stats may be null
  virtual int seed_centres(uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks, uint64_t* assign, vc_seed_stats* stats) = 0;
  // the k nearest label groups of every query, each by its member nearest to the query (vc_search_knn_distinct /
  // vc_sharded_search_knn_distinct): labels as any grouper above writes them, N entries; mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT;
  // k_first 0 = the default first k'; row_labels, counts and stats may be null; a count may carry VC_DISTINCT_TRUNCATED
  virtual int search_knn_distinct(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* labels, uint32_t k_first,
                                  uint64_t* out, uint32_t* row_labels, uint32_t* counts, vc_distinct_stats* stats) = 0;
  // the k nearest among the records a filter allows (vc_search_knn_filtered / vc_sharded_search_knn_filtered): sel and kind as
  // VC_FILTER_* reads them, one filter for the whole batch; mode VC_MODE_LINEAR or VC_MODE_MIH_EXACT; k_first 0 = the plan's first k';
  // counts and stats may be null; exact for every selectivity, counts = min(k, allowed)
  virtual int search_knn_filtered(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* sel, uint32_t kind, uint32_t value,
                                  uint32_t k_first, uint64_t* out, uint32_t* counts, vc_filter_stats* stats) = 0;
  // the k nearest inside each query's own scope (vc_search_knn_scoped / vc_sharded_search_knn_scoped): scope one word per record, qscope
  // one per query, a record counts for a query when the two words are equal; exact brute force, no mode; flags 0; counts and stats may
  // be null, counts = min(k, size of the query's scope)
  virtual int search_knn_scoped(const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope, const uint32_t* qscope, uint32_t flags,
                                uint64_t* out, uint32_t* counts, vc_scope_stats* stats) = 0;
  // the exact k-NN graph of the store (vc_knn_graph / vc_sharded_knn_graph): row p - first = the k nearest OTHER records of record
  // first + p as packed (dist << 32 | id), ascending, ties to the smaller id; count 0 = to the end; the same words in VC_MODE_LINEAR and
  // VC_MODE_MIH_EXACT; counts and stats may be null
  virtual int knn_graph(uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                        vc_knn_graph_stats* stats) = 0;
  // that graph after add_codes (vc_knn_graph_update / vc_sharded_knn_graph_update): rows has room for N * k words and counts (nullable)
  // for N, and their first n_old rows are knn_graph's over the store when it held its first n_old records; afterwards all N rows are
  // knn_graph's over the store now, the same words.  In VC_MODE_MIH_EXACT the index must be current (update_index)
  virtual int knn_graph_update(uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                               vc_knn_graph_update_stats* stats) = 0;
  // that graph after retain (vc_knn_graph_retain / vc_sharded_knn_graph_retain): rows [n_old][k] and counts (nullable) are knn_graph's
  // over the store before retain, new_ids the map retain wrote; afterwards the first K rows are knn_graph's over the store now, the same
  // words.  Only rows that lost too many entries are searched again
  virtual int knn_graph_retain(uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, uint64_t* rows,
                               uint32_t* counts, vc_knn_graph_retain_stats* stats) = 0;
  // components and in-degrees of that graph over the whole store (vc_cluster_knn / vc_sharded_cluster_knn): an edge is one of a row's
  // first kk entries at a distance <= max_dist; VC_KNN_MUTUAL joins two records iff each lists the other, VC_KNN_EITHER iff one does;
  // labels[i] = the smallest id of the component; counts, in_degree and stats may be null
  virtual int cluster_knn(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t* labels,
                          uint32_t* in_degree, vc_cluster_knn_stats* stats) = 0;
  // shared-nearest-neighbour clusters of that graph (vc_cluster_snn / vc_sharded_cluster_snn): a candidate pair (flags as cluster_knn)
  // is joined iff its two lists of kk share at least min_shared records; shared [N][kk] the weights (VC_SNN_NONE where nothing is
  // listed), hist [kk] their histogram; counts, shared, hist and stats may be null
  virtual int cluster_snn(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t min_shared,
                          uint32_t* labels, uint32_t* shared, uint64_t* hist, vc_cluster_snn_stats* stats) = 0;
  // that graph turned round, in CSR form (vc_knn_adjacency / vc_sharded_knn_adjacency): segment j = adj[offsets[j] .. offsets[j + 1])
  // holds dist << 32 | id, ascending, of every record that lists j (VC_KNN_REVERSE), that lists j and is listed by it (VC_KNN_MUTUAL)
  // or either (VC_KNN_EITHER); offsets has N + 1 words; VC_ERR_CAPACITY where offsets[N] > adj_cap (adj_cap 0 with a null adj sizes);
  // counts and stats may be null
  virtual int knn_adjacency(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint64_t* adj,
                            uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats) = 0;
  // the minimum spanning forest of that graph in Kruskal order (vc_knn_mst / vc_sharded_knn_mst): flags VC_KNN_MUTUAL / VC_KNN_EITHER,
  // weight_kind VC_MST_DISTANCE (min_pts 1) or VC_MST_REACHABILITY (min_pts in 1 .. k + 1); edges has room for max(N, 1) - 1 entries and
  // gets stats->n_tree of them, ascending in (weight, a, dist, b); labels [N], hist [bits + 1], counts and stats may be null
  virtual int knn_mst(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t weight_kind,
                      uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist, vc_knn_mst_stats* stats) = 0;
  // the components of the store under the edges of weight <= max_weight, smallest-id labels (vc_mst_cut / vc_sharded_mst_cut); any
  // edge list, sorted or not; n_clusters may be null
  virtual int mst_cut(const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters) = 0;
  // the HDBSCAN-style clusters of a spanning forest (vc_mst_condense / vc_sharded_mst_condense): the condensed tree at min_cluster_size, its
  // stabilities, the VC_CONDENSE_EOM or VC_CONDENSE_LEAF selection and the flat labels (own id = noise); nodes has room for max(N, 1) - 1
  // entries and gets stats->n_nodes of them; node, own and leave may be null
  virtual int mst_condense(const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method, vc_condensed_node* nodes,
                           uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave, vc_mst_condense_stats* stats) = 0;
  // the majority label among the first kk entries within max_dist of every row (vc_knn_vote / vc_sharded_knn_vote): rows are any rows
  // whose ids are resident (a graph, or a search's rows: the k-NN classifier), labels [N] with VC_VOTE_NONE for "unlabelled",
  // weight_kind VC_VOTE_COUNT / VC_VOTE_CLOSENESS; out_label [n_rows]; counts, out_votes, out_total and stats may be null
  virtual int knn_vote(const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist, const uint32_t* labels,
                       uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats) = 0;
  // synchronous label propagation over the CSR of knn_adjacency (vc_label_propagate / vc_sharded_label_propagate): flags 0 or
  // VC_LP_CLAMP_SEEDS, max_iters in 1 .. VC_LP_MAX_ITERS; labels_out [N]; votes, total [N] and stats may be null
  virtual int label_propagate(const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in, uint32_t weight_kind, uint32_t flags,
                              uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total, vc_label_propagate_stats* stats) = 0;
  // records taken out of the store and its index, the survivors renumbered in order (vc_retain / vc_sharded_retain; the reference has
  // no delete: this stands for build_hash_tables.cc run again over the code file without them).  kind VC_RETAIN_MASK / VC_RETAIN_ROOTS
  virtual int retain(const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) = 0;
};

// Owns one vc_engine (one shard / GPU).
class Engine : public Backend {
 public:
  Engine(uint32_t bits, uint32_t n_tables, uint64_t capacity, uint32_t flags = 0, uint32_t id_base = 0, int device = -1) {
    vc_config c{};
    c.abi_version = VC_ABI_VERSION;
    c.bits = bits;
    c.n_tables = n_tables;
    c.capacity = capacity;
    c.flags = flags;
    c.id_base = id_base;
    c.device = device;
    int rc = vc_create(&c, &h_);
    if (rc != VC_OK) throw EngineError(rc, vc_last_error(nullptr));
    bits_ = bits;
    m_ = n_tables;
  }
  ~Engine() override { vc_destroy(h_); }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  vc_engine* handle() const { return h_; }
  uint32_t bits() const override { return bits_; }
  uint32_t n_tables() const override { return m_; }
  const char* last_error() const override { return vc_last_error(h_); }
  int add_codes(const void* codes, uint64_t n) override { return vc_add_codes(h_, codes, n); }
  int load_code_file(const char* path, uint64_t max_records, uint64_t* n_read) override { return vc_load_code_file(h_, path, max_records, n_read); }
  int build_index() override { return vc_build_index(h_); }
  int update_index() override { return vc_update_index(h_); }
  uint64_t size() const override {
    uint64_t n = 0;
    vc_size(h_, &n);
    return n;
  }
  int get_code(uint32_t id, void* out) override { return vc_get_code(h_, id, out); }
  int get_bucket(uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n) override {
    return vc_get_bucket(h_, table, index, ids, codes, cap, n);
  }
  int search_knn(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint64_t* out, uint32_t* counts,
                 vc_query_stats* stats) override {
    return vc_search_knn(h_, queries, nq, k, mode, order, out, counts, stats);
  }
  int search_knn_ids(const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint32_t id_flags, uint64_t* out,
                     uint32_t* counts, vc_query_stats* stats) override {
    return vc_search_knn_ids(h_, ids, nq, k, mode, order, id_flags, out, counts, stats);
  }
  int search_radius_ids(const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags, uint64_t* out, uint64_t out_cap,
                        uint64_t* out_offsets) override {
    return vc_search_radius_ids(h_, ids, nq, radius, mode, id_flags, out, out_cap, out_offsets);
  }
  int cluster_radius(uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_cluster_stats* stats) override {
    return vc_cluster_radius(h_, radius, mode, batch, n_labelled, labels, stats);
  }
  int cluster_levels(uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_levels_stats* stats) override {
    return vc_cluster_levels(h_, max_radius, mode, batch, n_labelled, labels, stats);
  }
  int leaders_radius(uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_leader_stats* stats) override {
    return vc_leaders_radius(h_, radius, mode, batch, n_labelled, labels, stats);
  }
  int dbscan_radius(uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* degrees, vc_dbscan_stats* stats) override {
    return vc_dbscan_radius(h_, radius, min_pts, mode, batch, labels, degrees, stats);
  }
  int dbscan_levels(uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* core_dist, vc_dbscan_levels_stats* stats) override {
    return vc_dbscan_levels(h_, max_radius, min_pts, mode, batch, labels, core_dist, stats);
  }
  int group_summary(const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels, uint32_t* group_index,
                    uint64_t* n_groups) override {
    return vc_group_summary(h_, labels, groups_cap, groups, centroids, rep_labels, group_index, n_groups);
  }
  int assign_nearest(const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out) override {
    return vc_assign_nearest(h_, centres, n_centres, first, count, out);
  }
  int kmajority(uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels, vc_kmajority_stats* stats) override {
    return vc_kmajority(h_, n_centres, max_iters, centres, assign, labels, stats);
  }
  int seed_centres(uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks, uint64_t* assign, vc_seed_stats* stats) override {
    return vc_seed_centres(h_, n_centres, method, seed, centres, picks, assign, stats);
  }
  int search_knn_distinct(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* labels, uint32_t k_first,
                          uint64_t* out, uint32_t* row_labels, uint32_t* counts, vc_distinct_stats* stats) override {
    return vc_search_knn_distinct(h_, queries, nq, k, mode, order, labels, k_first, out, row_labels, counts, stats);
  }
  int search_knn_filtered(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* sel, uint32_t kind, uint32_t value,
                          uint32_t k_first, uint64_t* out, uint32_t* counts, vc_filter_stats* stats) override {
    return vc_search_knn_filtered(h_, queries, nq, k, mode, order, sel, kind, value, k_first, out, counts, stats);
  }
  int search_knn_scoped(const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope, const uint32_t* qscope, uint32_t flags,
                        uint64_t* out, uint32_t* counts, vc_scope_stats* stats) override {
    return vc_search_knn_scoped(h_, queries, nq, k, order, scope, qscope, flags, out, counts, stats);
  }
  int knn_graph(uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                vc_knn_graph_stats* stats) override {
    return vc_knn_graph(h_, k, mode, batch, first, count, k_first, rows, counts, stats);
  }
  int knn_graph_update(uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                       vc_knn_graph_update_stats* stats) override {
    return vc_knn_graph_update(h_, k, mode, batch, n_old, k_first, rows, counts, stats);
  }
  int knn_graph_retain(uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, uint64_t* rows, uint32_t* counts,
                       vc_knn_graph_retain_stats* stats) override {
    return vc_knn_graph_retain(h_, k, mode, batch, n_old, k_first, new_ids, rows, counts, stats);
  }
  int cluster_knn(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t* labels,
                  uint32_t* in_degree, vc_cluster_knn_stats* stats) override {
    return vc_cluster_knn(h_, rows, counts, k, kk, flags, max_dist, labels, in_degree, stats);
  }
  int cluster_snn(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t min_shared,
                  uint32_t* labels, uint32_t* shared, uint64_t* hist, vc_cluster_snn_stats* stats) override {
    return vc_cluster_snn(h_, rows, counts, k, kk, flags, max_dist, min_shared, labels, shared, hist, stats);
  }
  int knn_adjacency(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint64_t* adj,
                    uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats) override {
    return vc_knn_adjacency(h_, rows, counts, k, kk, flags, max_dist, adj, adj_cap, offsets, stats);
  }
  int knn_mst(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t weight_kind,
              uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist, vc_knn_mst_stats* stats) override {
    return vc_knn_mst(h_, rows, counts, k, kk, flags, max_dist, weight_kind, min_pts, edges, labels, hist, stats);
  }
  int mst_cut(const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters) override {
    return vc_mst_cut(h_, edges, n_edges, max_weight, labels, n_clusters);
  }
  int mst_condense(const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method, vc_condensed_node* nodes,
                   uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave, vc_mst_condense_stats* stats) override {
    return vc_mst_condense(h_, edges, n_edges, min_cluster_size, root_weight, method, nodes, labels, node, own, leave, stats);
  }
  int knn_vote(const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist, const uint32_t* labels,
               uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats) override {
    return vc_knn_vote(h_, rows, counts, n_rows, k, kk, max_dist, labels, weight_kind, out_label, out_votes, out_total, stats);
  }
  int label_propagate(const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in, uint32_t weight_kind, uint32_t flags,
                      uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total, vc_label_propagate_stats* stats) override {
    return vc_label_propagate(h_, offsets, adj, n_entries, labels_in, weight_kind, flags, max_iters, labels_out, votes, total, stats);
  }
  int retain(const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) override { return vc_retain(h_, sel, kind, new_ids, n_kept); }
 private:
  vc_engine* h_ = nullptr;
  uint32_t bits_ = 0, m_ = 0;
};

// The GPUs of one node behind the same interface (vc_sharded_*): the database split by id range into n_shards engines,
// one exchange of per-shard top-k per batch (RCCL all-gather over xGMI, or peer copies) + the merge kernel -- what the
// reference does with `mpirun -n 4` ranks, MPI_Gather/Gatherv/Bcast per radius and a master-side heap
// (run_distributed_search.py:74; search_worker.cc:99-101,177-207; mpi_coordinator.cc:26-69).
class ShardedEngine : public Backend {
 public:
  ShardedEngine(uint32_t bits, uint32_t n_tables, uint64_t capacity, uint32_t n_shards, const std::vector<int>& devices = {},
                uint32_t flags = 0, uint32_t id_base = 0, uint32_t exchange = VC_EXCHANGE_AUTO) {
    vc_sharded_config c{};
    c.abi_version = VC_ABI_VERSION;
    c.n_shards = n_shards;
    c.n_devices = (uint32_t)devices.size();
    c.exchange = exchange;
    for (size_t i = 0; i < devices.size() && i < VC_MAX_SHARDS; ++i) c.device_ids[i] = devices[i];
    c.engine.abi_version = VC_ABI_VERSION;
    c.engine.bits = bits;
    c.engine.n_tables = n_tables;
    c.engine.capacity = capacity;
    c.engine.flags = flags;
    c.engine.id_base = id_base;
    c.engine.device = -1;
    int rc = vc_sharded_create(&c, &h_);
    if (rc != VC_OK) throw EngineError(rc, vc_sharded_last_error(nullptr));
    bits_ = bits;
    m_ = n_tables;
  }
  ~ShardedEngine() override { vc_sharded_destroy(h_); }
  ShardedEngine(const ShardedEngine&) = delete;
  ShardedEngine& operator=(const ShardedEngine&) = delete;
  vc_sharded* handle() const { return h_; }
  uint32_t bits() const override { return bits_; }
  uint32_t n_tables() const override { return m_; }
  const char* last_error() const override { return vc_sharded_last_error(h_); }
  int add_codes(const void* codes, uint64_t n) override { return vc_sharded_add_codes(h_, codes, n); }
  int load_code_file(const char* path, uint64_t max_records, uint64_t* n_read) override {   // build_hash_tables.cc:40-70
    FILE* fh = fopen(path, "rb");
    if (!fh) return VC_ERR_INVALID;
    const size_t rec = nbytes(), batch = (size_t)1 << 16;
    std::vector<char> buf(rec * batch);
    uint64_t total = 0;
    int rc = VC_OK;
    while (max_records == 0 || total < max_records) {
      const size_t want = max_records ? (size_t)std::min<uint64_t>(batch, max_records - total) : batch;
      const size_t got = fread(buf.data(), rec, want, fh);
      if (got == 0) break;
      if ((rc = vc_sharded_add_codes(h_, buf.data(), got))) break;
      total += got;
    }
    fclose(fh);
    if (n_read) *n_read = total;
    return rc;
  }
  int build_index() override { return vc_sharded_build_index(h_); }
  int update_index() override { return vc_sharded_update_index(h_); }
  uint64_t size() const override {
    uint64_t n = 0;
    vc_sharded_size(h_, &n);
    return n;
  }
  int get_code(uint32_t id, void* out) override { return vc_sharded_get_code(h_, id, out); }
  int get_bucket(uint32_t table, uint32_t index, uint32_t* ids, void* codes, uint32_t cap, uint32_t* n) override {
    return vc_sharded_get_bucket(h_, table, index, ids, codes, cap, n);
  }
  int search_knn(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint64_t* out, uint32_t* counts,
                 vc_query_stats* stats) override {
    return vc_sharded_search_knn(h_, queries, nq, k, mode, order, out, counts, stats);
  }
  int search_knn_ids(const uint32_t* ids, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, uint32_t id_flags, uint64_t* out,
                     uint32_t* counts, vc_query_stats* stats) override {
    return vc_sharded_search_knn_ids(h_, ids, nq, k, mode, order, id_flags, out, counts, stats);
  }
  int search_radius_ids(const uint32_t* ids, uint32_t nq, uint32_t radius, uint32_t mode, uint32_t id_flags, uint64_t* out, uint64_t out_cap,
                        uint64_t* out_offsets) override {
    return vc_sharded_search_radius_ids(h_, ids, nq, radius, mode, id_flags, out, out_cap, out_offsets);
  }
  int cluster_radius(uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_cluster_stats* stats) override {
    return vc_sharded_cluster_radius(h_, radius, mode, batch, n_labelled, labels, stats);
  }
  int cluster_levels(uint32_t max_radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_levels_stats* stats) override {
    return vc_sharded_cluster_levels(h_, max_radius, mode, batch, n_labelled, labels, stats);
  }
  int leaders_radius(uint32_t radius, uint32_t mode, uint32_t batch, uint64_t n_labelled, uint32_t* labels, vc_leader_stats* stats) override {
    return vc_sharded_leaders_radius(h_, radius, mode, batch, n_labelled, labels, stats);
  }
  int dbscan_radius(uint32_t radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* degrees, vc_dbscan_stats* stats) override {
    return vc_sharded_dbscan_radius(h_, radius, min_pts, mode, batch, labels, degrees, stats);
  }
  int dbscan_levels(uint32_t max_radius, uint32_t min_pts, uint32_t mode, uint32_t batch, uint32_t* labels, uint32_t* core_dist, vc_dbscan_levels_stats* stats) override {
    return vc_sharded_dbscan_levels(h_, max_radius, min_pts, mode, batch, labels, core_dist, stats);
  }
  int group_summary(const uint32_t* labels, uint64_t groups_cap, vc_group* groups, void* centroids, uint32_t* rep_labels, uint32_t* group_index,
                    uint64_t* n_groups) override {
    return vc_sharded_group_summary(h_, labels, groups_cap, groups, centroids, rep_labels, group_index, n_groups);
  }
  int assign_nearest(const void* centres, uint32_t n_centres, uint64_t first, uint64_t count, uint64_t* out) override {
    return vc_sharded_assign_nearest(h_, centres, n_centres, first, count, out);
  }
  int kmajority(uint32_t n_centres, uint32_t max_iters, void* centres, uint64_t* assign, uint32_t* labels, vc_kmajority_stats* stats) override {
    return vc_sharded_kmajority(h_, n_centres, max_iters, centres, assign, labels, stats);
  }
  int seed_centres(uint32_t n_centres, uint32_t method, uint64_t seed, void* centres, uint64_t* picks, uint64_t* assign, vc_seed_stats* stats) override {
    return vc_sharded_seed_centres(h_, n_centres, method, seed, centres, picks, assign, stats);
  }
  int search_knn_distinct(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* labels, uint32_t k_first,
                          uint64_t* out, uint32_t* row_labels, uint32_t* counts, vc_distinct_stats* stats) override {
    return vc_sharded_search_knn_distinct(h_, queries, nq, k, mode, order, labels, k_first, out, row_labels, counts, stats);
  }
  int search_knn_filtered(const void* queries, uint32_t nq, uint32_t k, uint32_t mode, uint32_t order, const uint32_t* sel, uint32_t kind, uint32_t value,
                          uint32_t k_first, uint64_t* out, uint32_t* counts, vc_filter_stats* stats) override {
    return vc_sharded_search_knn_filtered(h_, queries, nq, k, mode, order, sel, kind, value, k_first, out, counts, stats);
  }
  int search_knn_scoped(const void* queries, uint32_t nq, uint32_t k, uint32_t order, const uint32_t* scope, const uint32_t* qscope, uint32_t flags,
                        uint64_t* out, uint32_t* counts, vc_scope_stats* stats) override {
    return vc_sharded_search_knn_scoped(h_, queries, nq, k, order, scope, qscope, flags, out, counts, stats);
  }
  int knn_graph(uint32_t k, uint32_t mode, uint32_t batch, uint64_t first, uint64_t count, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                vc_knn_graph_stats* stats) override {
    return vc_sharded_knn_graph(h_, k, mode, batch, first, count, k_first, rows, counts, stats);
  }
  int knn_graph_update(uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, uint64_t* rows, uint32_t* counts,
                       vc_knn_graph_update_stats* stats) override {
    return vc_sharded_knn_graph_update(h_, k, mode, batch, n_old, k_first, rows, counts, stats);
  }
  int knn_graph_retain(uint32_t k, uint32_t mode, uint32_t batch, uint64_t n_old, uint32_t k_first, const uint32_t* new_ids, uint64_t* rows, uint32_t* counts,
                       vc_knn_graph_retain_stats* stats) override {
    return vc_sharded_knn_graph_retain(h_, k, mode, batch, n_old, k_first, new_ids, rows, counts, stats);
  }
  int cluster_knn(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t* labels,
                  uint32_t* in_degree, vc_cluster_knn_stats* stats) override {
    return vc_sharded_cluster_knn(h_, rows, counts, k, kk, flags, max_dist, labels, in_degree, stats);
  }
  int cluster_snn(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t min_shared,
                  uint32_t* labels, uint32_t* shared, uint64_t* hist, vc_cluster_snn_stats* stats) override {
    return vc_sharded_cluster_snn(h_, rows, counts, k, kk, flags, max_dist, min_shared, labels, shared, hist, stats);
  }
  int knn_adjacency(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint64_t* adj,
                    uint64_t adj_cap, uint64_t* offsets, vc_knn_adjacency_stats* stats) override {
    return vc_sharded_knn_adjacency(h_, rows, counts, k, kk, flags, max_dist, adj, adj_cap, offsets, stats);
  }
  int knn_mst(const uint64_t* rows, const uint32_t* counts, uint32_t k, uint32_t kk, uint32_t flags, uint32_t max_dist, uint32_t weight_kind,
              uint32_t min_pts, vc_mst_edge* edges, uint32_t* labels, uint64_t* hist, vc_knn_mst_stats* stats) override {
    return vc_sharded_knn_mst(h_, rows, counts, k, kk, flags, max_dist, weight_kind, min_pts, edges, labels, hist, stats);
  }
  int mst_cut(const vc_mst_edge* edges, uint64_t n_edges, uint32_t max_weight, uint32_t* labels, uint64_t* n_clusters) override {
    return vc_sharded_mst_cut(h_, edges, n_edges, max_weight, labels, n_clusters);
  }
  int mst_condense(const vc_mst_edge* edges, uint64_t n_edges, uint32_t min_cluster_size, uint32_t root_weight, uint32_t method, vc_condensed_node* nodes,
                   uint32_t* labels, uint32_t* node, uint32_t* own, uint32_t* leave, vc_mst_condense_stats* stats) override {
    return vc_sharded_mst_condense(h_, edges, n_edges, min_cluster_size, root_weight, method, nodes, labels, node, own, leave, stats);
  }
  int knn_vote(const uint64_t* rows, const uint32_t* counts, uint64_t n_rows, uint32_t k, uint32_t kk, uint32_t max_dist, const uint32_t* labels,
               uint32_t weight_kind, uint32_t* out_label, uint32_t* out_votes, uint32_t* out_total, vc_knn_vote_stats* stats) override {
    return vc_sharded_knn_vote(h_, rows, counts, n_rows, k, kk, max_dist, labels, weight_kind, out_label, out_votes, out_total, stats);
  }
  int label_propagate(const uint64_t* offsets, const uint64_t* adj, uint64_t n_entries, const uint32_t* labels_in, uint32_t weight_kind, uint32_t flags,
                      uint32_t max_iters, uint32_t* labels_out, uint32_t* votes, uint32_t* total, vc_label_propagate_stats* stats) override {
    return vc_sharded_label_propagate(h_, offsets, adj, n_entries, labels_in, weight_kind, flags, max_iters, labels_out, votes, total, stats);
  }
  int retain(const uint32_t* sel, uint32_t kind, uint32_t* new_ids, uint64_t* n_kept) override { return vc_sharded_retain(h_, sel, kind, new_ids, n_kept); }
 private:
  vc_sharded* h_ = nullptr;
  uint32_t bits_ = 0, m_ = 0;
};

// VC_SHARDS=G [VC_DEVICES=0,1,...]: the drivers' switch from one engine to the sharded store (no argv position is free for
// it: run_distributed_search.py:74-79 fixes them all).  G = 1 (or unset) is the one-GPU Engine -- a one-shard store would
// only add an exchange, a merge and copies --; anything that is not a number in 1..VC_MAX_SHARDS is refused, not guessed at.
// Under VC_SHARDS every shard stops by its own rule unless VC_GLOBAL_STOP=1: then the exact search stops where one
// SearchWorker over the whole database stops (VC_FLAG_GLOBAL_STOP, verticut_gpu.h) and prints its rows and statistics.
// Without it the printed n_sub_reads / n_local_reads are SUMS over the shards and radius the widest shard's.
// VC_GLOBAL_STOP=1 with VC_REF_QUIRKS=1 is refused: the reference's quirks make its radius loop inexact.
// VC_GLOBAL_APPROX=1 does the same for the approximate search (VC_FLAG_GLOBAL_APPROX): one heap of 20 k distinct candidates over
// all shards, as the reference's master fills it (search_worker.cc:104-139).  It may be combined with VC_REF_QUIRKS=1.
inline Backend* make_backend(uint32_t bits, uint32_t n_tables, uint64_t capacity, uint32_t flags) {
  const char* g = getenv("VC_SHARDS");
  long shards = 1;
  if (g && *g) {
    char* end = nullptr;
    shards = strtol(g, &end, 10);
    if (end == g || *end != '\0' || shards < 1 || shards > VC_MAX_SHARDS)
      throw EngineError(VC_ERR_INVALID, std::string("VC_SHARDS must be a number in 1..") + std::to_string(VC_MAX_SHARDS) + ", got '" + g + "'");
  }
  const char* gs = getenv("VC_GLOBAL_STOP");
  if (gs && atoi(gs)) {
    if (flags & (VC_FLAG_REF_SIGNEXT_KEYS | VC_FLAG_REF_STOP_LITERAL4))
      throw EngineError(VC_ERR_INVALID, "VC_GLOBAL_STOP=1 cannot be combined with VC_REF_QUIRKS=1 (the quirks make the radius loop inexact)");
    flags |= VC_FLAG_GLOBAL_STOP;   // a one-GPU Engine ignores it: its stop is global already
  }
  const char* ga = getenv("VC_GLOBAL_APPROX");
  if (ga && atoi(ga)) flags |= VC_FLAG_GLOBAL_APPROX;   // (ignored by a one-GPU Engine as well)
  if (shards <= 1) return new Engine(bits, n_tables, capacity, flags);
  std::vector<int> devices;
  if (const char* d = getenv("VC_DEVICES"))
    for (const char* p = d; *p;) {
      char* end = nullptr;
      const long v = strtol(p, &end, 10);
      if (end == p || v < 0 || (*end != ',' && *end != '\0'))
        throw EngineError(VC_ERR_INVALID, std::string("VC_DEVICES must be comma-separated device ordinals, got '") + d + "'");
      devices.push_back((int)v);
      p = *end == ',' ? end + 1 : end;
    }
  return new ShardedEngine(bits, n_tables, capacity, (uint32_t)shards, devices, flags);
}

// BaseProxy over the resident index.  put(ID, BinaryCode) appends a record (ids must arrive in order, as
// build_hash_tables.cc:55-69 produces them); put(HashIndex, Image_List) is accepted and ignored because the
// buckets are derived from the records (rule a12): by Backend::build_index from all of them, or by
// Backend::update_index, which appends the records put since the last build / update to their buckets -- the
// reference's get bucket / append / put (build_hash_tables.cc:40-70), done for a whole batch of puts in one
// merge.  Between a put and the next update_index / build_index, get(HashIndex) fails (the index is stale).
class GpuProxy : public BaseProxy<Message, Message> {
 public:
  explicit GpuProxy(Backend* e) : e_(e) {}
  int init(const char*) override { return 0; }   // pilaf_proxy.h:65-80 reads a host list; nothing to connect to here
  void close() override {}
  int contain(const Message&) override { return PROXY_NOT_FOUND; }  // unimplemented in every reference proxy too

  int get(const Message& key, Message& value) override {
    if (const HashIndex* hi = dynamic_cast<const HashIndex*>(&key)) {
      Image_List* out = dynamic_cast<Image_List*>(&value);
      if (!out) return PROXY_NOT_FOUND;
      out->clear_images();
      uint32_t n = 0;
      int rc = e_->get_bucket(hi->table_id(), hi->index(), nullptr, nullptr, 0, &n);
      if (rc == VC_NOT_FOUND) return PROXY_NOT_FOUND;
      e_->check(rc);
      std::vector<uint32_t> ids(n);
      std::string codes((size_t)n * e_->nbytes(), '\0');
      e_->check(e_->get_bucket(hi->table_id(), hi->index(), ids.data(), &codes[0], n, &n));
      for (uint32_t i = 0; i < n; ++i) {
        ID_Code_Pair* p = out->add_images();
        p->set_id(ids[i]);
        p->set_code(codes.data() + (size_t)i * e_->nbytes(), e_->nbytes());
      }
      return PROXY_FOUND;
    }
    if (const ID* id = dynamic_cast<const ID*>(&key)) {
      BinaryCode* out = dynamic_cast<BinaryCode*>(&value);
      if (!out) return PROXY_NOT_FOUND;
      std::string buf(e_->nbytes(), '\0');
      int rc = e_->get_code(id->id(), &buf[0]);
      if (rc == VC_NOT_FOUND) return PROXY_NOT_FOUND;
      e_->check(rc);
      out->set_code(buf.data(), buf.size());
      return PROXY_FOUND;
    }
    return PROXY_NOT_FOUND;
  }

  int put(const Message& key, const Message& value) override {
    if (const ID* id = dynamic_cast<const ID*>(&key)) {
      const BinaryCode* c = dynamic_cast<const BinaryCode*>(&value);
      const uint64_t n = e_->size();
      if (!c || c->code().size() != e_->nbytes() || id->id() != n) return PROXY_PUT_FAIL;
      return e_->add_codes(c->code().data(), 1) == VC_OK ? PROXY_PUT_DONE : PROXY_PUT_FAIL;
    }
    if (dynamic_cast<const HashIndex*>(&key)) return PROXY_PUT_DONE;
    return PROXY_PUT_FAIL;
  }

 private:
  Backend* e_;
};

// ---- src/search_worker.h:18-64
class SearchWorker {
 public:
  struct search_result_st {
    uint32_t image_id;
    uint32_t dist;
  };

  // The reference takes (mpi_coordinator*, BaseProxy*, image_total); the coordinator is gone (all tables
  // live in one HBM), the proxy's engine is what is searched.
  SearchWorker(Backend* engine, int image_total) : e_(engine), image_total_(image_total) {}

  // search_worker.cc:65-89.  approximate -> search_K_approximate_nearest_neighbors (:93-157),
  // else search_K_nearest_neighbors (:159-218).  Farthest first, like the reference's heap drain.
  std::list<search_result_st> find(const char* binary_code, size_t nbytes, int knn, bool approximate) {
    if (nbytes != e_->nbytes() || e_->n_tables() == 0 || nbytes % e_->n_tables() != 0)   // :75 assert
      throw EngineError(VC_ERR_INVALID, "find: nbytes must equal the engine's code size and divide by n_tables");
    result_.clear();
    std::vector<uint64_t> out((size_t)knn);
    uint32_t cnt = 0;
    e_->check(e_->search_knn(binary_code, 1, (uint32_t)knn, approximate ? VC_MODE_MIH_APPROX : VC_MODE_MIH_EXACT,
                             VC_ORDER_FARTHEST_FIRST, out.data(), &cnt, &stat_));
    for (uint32_t i = 0; i < cnt; ++i) result_.push_back({(uint32_t)(out[i] & 0xffffffffu), (uint32_t)(out[i] >> 32)});
    return result_;
  }
  // The same for a BATCH of queries in one ABI call (n_query codes of nbytes each, back to back): the reference's drivers
  // call find() once per query (distributed_image_search.cc:62-85, accuracy_test.cc:72-91); on the GPU a batch shares every
  // launch, so 200 queries cost little more than one.  Results and per-query statistics exactly as n_query find() calls.
  std::vector<std::list<search_result_st> > find_batch(const char* binary_codes, size_t nbytes, uint32_t n_query, int knn,
                                                       bool approximate, std::vector<vc_query_stats>* stats = nullptr) {
    if (nbytes != e_->nbytes() || e_->n_tables() == 0 || nbytes % e_->n_tables() != 0)   // :75 assert
      throw EngineError(VC_ERR_INVALID, "find: nbytes must equal the engine's code size and divide by n_tables");
    std::vector<std::list<search_result_st> > all(n_query);
    if (n_query == 0) return all;
    std::vector<uint64_t> out((size_t)n_query * knn);
    std::vector<uint32_t> cnt(n_query);
    std::vector<vc_query_stats> st(n_query);
    e_->check(e_->search_knn(binary_codes, n_query, (uint32_t)knn, approximate ? VC_MODE_MIH_APPROX : VC_MODE_MIH_EXACT,
                             VC_ORDER_FARTHEST_FIRST, out.data(), cnt.data(), st.data()));
    for (uint32_t q = 0; q < n_query; ++q)
      for (uint32_t i = 0; i < cnt[q]; ++i) {
        const uint64_t v = out[(size_t)q * knn + i];
        all[q].push_back({(uint32_t)(v & 0xffffffffu), (uint32_t)(v >> 32)});
      }
    result_ = all.back();
    stat_ = st.back();
    if (stats) *stats = st;
    return all;
  }
  std::list<search_result_st> get_knn() { return result_; }
  // search_worker.cc:24-30
  void get_stat(uint64_t& n_main_reads, uint64_t& n_sub_reads, uint64_t& n_local_reads, uint32_t& radius) {
    n_main_reads = stat_.n_main_reads;
    n_sub_reads = stat_.n_sub_reads;
    n_local_reads = stat_.n_local_reads;
    radius = stat_.radius;
  }

  // linear_search.cc:39-64 as a member (the reference keeps it as a free function over globals)
  std::list<search_result_st> linear_search(const char* binary_code, int knn) {
    std::vector<uint64_t> out((size_t)knn);
    uint32_t cnt = 0;
    e_->check(e_->search_knn(binary_code, 1, (uint32_t)knn, VC_MODE_LINEAR, VC_ORDER_FARTHEST_FIRST, out.data(), &cnt, nullptr));
    std::list<search_result_st> r;
    for (uint32_t i = 0; i < cnt; ++i) r.push_back({(uint32_t)(out[i] & 0xffffffffu), (uint32_t)(out[i] >> 32)});
    return r;
  }

 private:
  Backend* e_;
  int image_total_;
  std::list<search_result_st> result_;
  vc_query_stats stat_{};
};

// ---- src/image_search_client.h:12-27 (served in process: image_search_server.cc:22-102 without ssh/popen)
class image_search_client {
 public:
  explicit image_search_client(Backend* engine) : e_(engine), worker_(engine, 0) {}
  std::string ping(const std::string& s) { return s; }   // image_search_server.cc:51-53 echoes the string
  // (image id, distance) pairs in the order the worker prints them ("id : dist" lines, farthest first).
  // The by-id path is dead in the reference as shipped (distributed_image_search.cc:116); here the code of
  // image `id` is read back from the resident DB and searched.
  std::list<std::pair<uint32_t, uint32_t> > search_image_by_id(uint32_t id, int knn, bool approximate = false) {
    std::string code(e_->nbytes(), '\0');
    int rc = e_->get_code(id, &code[0]);
    if (rc == VC_NOT_FOUND) throw EngineError(VC_NOT_FOUND, "Can't find match");   // distributed_image_search.cc:98
    e_->check(rc);
    std::list<std::pair<uint32_t, uint32_t> > out;
    for (const auto& r : worker_.find(code.data(), code.size(), knn, approximate)) out.push_back({r.image_id, r.dist});
    return out;
  }
  // The same for a BATCH of ids in one ABI call (what image_search_test.cc:112-170 replays one id at a time): one
  // farthest-first list per id, as search_image_by_id returns it; an id that is not in the database gives an empty list
  // instead of an exception.  The codes are gathered on the device, so 4 096 ids cost little more than one.
  std::vector<std::list<std::pair<uint32_t, uint32_t> > > search_images_by_id(const std::vector<uint32_t>& ids, int knn,
                                                                              bool approximate = false) {
    std::vector<std::list<std::pair<uint32_t, uint32_t> > > all(ids.size());
    if (ids.empty()) return all;
    const uint32_t nq = (uint32_t)ids.size();
    std::vector<uint64_t> out((size_t)nq * knn);
    std::vector<uint32_t> cnt(nq);
    e_->check(e_->search_knn_ids(ids.data(), nq, (uint32_t)knn, approximate ? VC_MODE_MIH_APPROX : VC_MODE_MIH_EXACT,
                                 VC_ORDER_FARTHEST_FIRST, 0, out.data(), cnt.data(), nullptr));
    for (uint32_t q = 0; q < nq; ++q)
      for (uint32_t i = 0; i < cnt[q]; ++i) {
        const uint64_t v = out[(size_t)q * knn + i];
        all[q].push_back({(uint32_t)(v & 0xffffffffu), (uint32_t)(v >> 32)});
      }
    return all;
  }
  // "Which images lie within `radius` of image `id`": (image id, distance) pairs formed as search_image_by_id forms them, NEAREST
  // first; by default without the image itself (VC_IDS_ONLY_GREATER lists every pair of a walk over all ids once).  Exact: MIH where
  // the store has tables, else the linear scan.  An id that is not in the database gives an empty list.
  std::list<std::pair<uint32_t, uint32_t> > search_image_by_id_within(uint32_t id, uint32_t radius, uint32_t id_flags = VC_IDS_EXCLUDE_SELF) {
    const uint32_t mode = e_->n_tables() ? VC_MODE_MIH_EXACT : VC_MODE_LINEAR;
    uint64_t offs[2] = {0, 0};
    std::vector<uint64_t> res;
    int rc = e_->search_radius_ids(&id, 1, radius, mode, id_flags, nullptr, 0, offs);   // the size first
    if (rc == VC_ERR_CAPACITY) {
      res.resize(offs[1]);
      rc = e_->search_radius_ids(&id, 1, radius, mode, id_flags, res.data(), res.size(), offs);
    }
    e_->check(rc);
    std::list<std::pair<uint32_t, uint32_t> > out;
    for (uint64_t i = offs[0]; i < offs[1]; ++i) out.push_back({(uint32_t)(res[i] & 0xffffffffu), (uint32_t)(res[i] >> 32)});
    return out;
  }
 private:
  Backend* e_;
  SearchWorker worker_;
};

}  // namespace vc
