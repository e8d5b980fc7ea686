// Native host implementation of the multibridged de-Bruijn graph of one partition (rows a12-a24):
// the same algorithm as shannon_amd/mbgraph.py (itself the index-based mirror of the reference's
// multibridging.py:145-325 + mbgraph.py), in C++ because at realistic coverage the per-partition
// graph surgery in Python was 2/3 of the whole step.  Control logic over small irregular graphs:
// host code; the order-defining conventions (P1-P3) are identical to the Python mirror,
// which stays as the readable specification and is cross-checked against this in the tests.
// (mbgraph_reads.h brings common.h, flatmap.h and graph_dev.h, and -- beside the reads -- what both sides of the stage share: the
// host-thread budget ThreadBudget / BudgetGuard / FreeThreads, run_on_threads, the clock tnow, the lap printer lap_line, base_code)
#include "mbgraph_reads.h"
#include "unitigs.h"
#include "graph_result.h"
#include <unordered_map>
#include <map>
#include <set>
#include <cmath>
#include <array>
#include <cstdlib>

namespace {

typedef std::pair<int, int> RI;   // (read id, index)

// unique packed K-mer keys -> groups of occurrences (kept in insertion order inside a group)
struct SeedIndex {
  std::vector<uint64_t> keys;               // sorted unique
  std::vector<uint32_t> goff;               // CSR into occ
  std::vector<std::pair<int, int>> occ;     // (node, offset)
  void build(std::vector<std::pair<uint64_t, std::pair<int, int>>>& items) {
    std::stable_sort(items.begin(), items.end(), [](const std::pair<uint64_t, std::pair<int, int>>& a, const std::pair<uint64_t, std::pair<int, int>>& b) { return a.first < b.first; });
    keys.clear(); goff.clear(); occ.clear();
    for (size_t i = 0; i < items.size(); i++) {
      if (i == 0 || items[i].first != items[i - 1].first) { keys.push_back(items[i].first); goff.push_back((uint32_t)occ.size()); }
      occ.push_back(items[i].second);
    }
    goff.push_back((uint32_t)occ.size());
  }
  int find(uint64_t key) const {
    auto it = std::lower_bound(keys.begin(), keys.end(), key);
    return (it != keys.end() && *it == key) ? (int)(it - keys.begin()) : -1;
  }
};

// ascending order for a list that is usually ascending already or two ascending runs one after the other (a bridging step hands a
// new node the reads of the old one twice, each time in order): a merge instead of a sort
template <class V> static void sort_runs(V& v) {
  auto b = v.begin(), e = v.end();
  auto p = std::is_sorted_until(b, e);
  if (p == e) return;
  if (std::is_sorted(p, e)) { std::inplace_merge(b, p, e); return; }
  std::sort(b, e);
}

struct Graph {
  bool laps = false;                        // print the time of every phase (SHN_DEBUG / SHN_GRAPH_LAPS)
  shn_ctx* ctx = nullptr;                   // non-NULL: K-mer seed scans run on the GPU (csrc/seeds.hip)
  int K, L, SIZE_THRESHOLD;
  std::vector<std::string> bases;
  std::vector<std::vector<int>> ine, oute;
  std::vector<double> norm, cc, prev, cnt;
  std::vector<char> cc_int;
  std::vector<char> dead;
  std::vector<std::vector<RI>> nreads;
  std::vector<signed char> bridged;   // -1 None, 0 False, 1 True
  std::vector<int> hash;
  std::vector<int> order;
  std::vector<int> es, ed, ew;
  std::vector<double> ecc;
  PartitionReads reads;                    // the partition's reads: text, copies, mates, first / last nodes (mbgraph_reads.h)
  shn_kp* kp = nullptr;
  std::vector<uint32_t> mate_cand;                  // (a, b) node pairs of find_mate_pairs' pass over the reads, made on the device
  bool mate_cand_ready = false;
  int attrs_rc = 0;                                 // a failed fetch of the host arrays (find_known_paths is void)
  ~Graph() { if (kp) shn_kp_destroy(kp); }
  std::set<std::vector<int>> known_paths;
  std::map<std::pair<int, int>, double> known_edges;
  std::vector<int> bridged_log;
  int n_known = 0, n_mate = 0;
  int nodes_after[4] = {0, 0, 0, 0};  // condensing, suspicious, collapse, bridging
  int final_nodes = 0;
  bool precondensed = false;          // loaded from GPU unitigs: the first condense_all is already done

  int new_node(const std::string& b) {
    int n = (int)bases.size();
    bases.push_back(b);
    ine.emplace_back(); oute.emplace_back();
    norm.push_back(1.0); cc.push_back(0.0); prev.push_back(0.0); cnt.push_back(1.0); cc_int.push_back(0);
    dead.push_back(0); nreads.emplace_back(); bridged.push_back(-1); hash.push_back(-2);
    order.push_back(n);
    return n;
  }
  void reserve_nodes(size_t n) {
    bases.reserve(n); ine.reserve(n); oute.reserve(n); norm.reserve(n); cc.reserve(n); prev.reserve(n); cnt.reserve(n);
    cc_int.reserve(n); dead.reserve(n); nreads.reserve(n); bridged.reserve(n); hash.reserve(n); order.reserve(n);
  }
  int link(int a, int b, int w) {
    int e = (int)es.size();
    es.push_back(a); ed.push_back(b); ew.push_back(w); ecc.push_back(0.0);
    oute[a].push_back(e); ine[b].push_back(e);
    return e;
  }
  static void erase_first(std::vector<int>& v, int x) {
    auto it = std::find(v.begin(), v.end(), x);
    if (it != v.end()) v.erase(it);
  }
  void kill_edge(int e) {
    erase_first(oute[es[e]], e);
    erase_first(ine[ed[e]], e);
    es[e] = -1; ed[e] = -1;
  }
  void kill_node(int n) { dead[n] = 1; }
  void full_destroy(int n) {
    std::vector<int> a = ine[n];
    for (int e : a) kill_edge(e);
    std::vector<int> b = oute[n];
    for (int e : b) kill_edge(e);
    nreads[n].clear();
    kill_node(n);
  }
  void remove_destroyed() {
    std::vector<int> o;
    o.reserve(order.size());
    for (int n : order) if (!dead[n]) o.push_back(n);
    order.swap(o);
  }
  std::vector<int> succ(int n) const { std::vector<int> r; for (int e : oute[n]) r.push_back(ed[e]); return r; }
  std::vector<int> pred(int n) const { std::vector<int> r; for (int e : ine[n]) r.push_back(es[e]); return r; }
  bool is_xnode(int n) const { return ine[n].size() >= 2 && oute[n].size() >= 2; }
  double avg_prev(int n) const { return prev[n] / cnt[n]; }

  // ---- loading (multibridging.py:145-172, 22-30, 68-97; mbgraph.py:44-62)
  void load_k1mers(const uint8_t* rows, uint64_t n_rows) {
    StringInterner idx(n_rows * 2);               // K-mer -> node (node ids == intern ids: nodes are only made here)
    idx.arena.reserve(n_rows * (size_t)K * 5 / 4);
    const int k1 = K + 1;
    reserve_nodes(n_rows * 5 / 2);
    es.reserve(n_rows * 4); ed.reserve(n_rows * 4); ew.reserve(n_rows * 4); ecc.reserve(n_rows * 4);
    for (uint64_t i = 0; i < n_rows; i++) {
      const char* km = (const char*)rows + i * k1;
      bool fresh;
      int na = idx.intern(km, K, &fresh);
      if (fresh) new_node(std::string(km, K));
      int nb = idx.intern(km + 1, K, &fresh);
      if (fresh) new_node(std::string(km + 1, K));
      link(na, nb, K - 1);
    }
    for (int n : order) { double s = 0; for (int e : oute[n]) s += ew[e]; prev[n] = s; }
  }
  // The same state as load_k1mers + the first condense_all, from the unitigs the GPU contracted (csrc/graph_gpu.hip): final
  // nodes in creation order, edges in id order, every node's out-/in-list in the order the sequential merges leave it.
  // bases / base_off: the partition's nodes; n_len = K-mers per node; tail_out = out-degree of the node's last K-mer.
  void load_unitigs(const char* ub, const uint64_t* base_off, const uint32_t* n_len, const uint32_t* tail_out, uint64_t n_nodes,
                    const uint32_t* e_src, const uint32_t* e_dst, const uint32_t* e_out_rank, const uint32_t* e_in_rank, uint64_t n_edges) {
    reserve_nodes(n_nodes * 2 + 16);
    es.reserve(n_edges * 3); ed.reserve(n_edges * 3); ew.reserve(n_edges * 3); ecc.reserve(n_edges * 3);
    for (uint64_t i = 0; i < n_nodes; i++) {
      const int n = new_node(std::string(ub + base_off[i], base_off[i + 1] - base_off[i]));
      const double m = (double)n_len[i];
      cnt[n] = m; norm[n] = m;                                       // sums of the K-mers' 1.0s
      prev[n] = (double)(K - 1) * ((m - 1.0) + (double)tail_out[i]);  // sum of (K-1) * out-degree over the K-mers (multibridging.py:169 quirk)
    }
    std::vector<uint32_t> odeg(n_nodes, 0), ideg(n_nodes, 0);
    for (uint64_t x = 0; x < n_edges; x++) { odeg[e_src[x]]++; ideg[e_dst[x]]++; }
    for (uint64_t i = 0; i < n_nodes; i++) { oute[i].assign(odeg[i], -1); ine[i].assign(ideg[i], -1); }
    for (uint64_t x = 0; x < n_edges; x++) {
      const int e = (int)es.size();
      es.push_back((int)e_src[x]); ed.push_back((int)e_dst[x]); ew.push_back(K - 1); ecc.push_back(0.0);
      oute[e_src[x]][e_out_rank[x]] = e;
      ine[e_dst[x]][e_in_rank[x]] = e;
    }
  }
  // order-sensitive signature of the graph (development check of load_unitigs against load_k1mers + condense_all)
  std::string signature() const {
    std::vector<int> idx(bases.size(), -1);
    for (size_t i = 0; i < order.size(); i++) idx[order[i]] = (int)i;
    std::string sg;
    char buf[96];
    for (int n : order) {
      sg += bases[n];
      snprintf(buf, sizeof buf, "|%.17g|%.17g|%.17g|%.17g|o", cnt[n], prev[n], norm[n], cc[n]);
      sg += buf;
      for (int e : oute[n]) { snprintf(buf, sizeof buf, " %d:%d", idx[ed[e]], ew[e]); sg += buf; }
      sg += "|i";
      for (int e : ine[n]) { snprintf(buf, sizeof buf, " %d:%d", idx[es[e]], ew[e]); sg += buf; }
      sg += "\n";
    }
    // edge ids in creation order (relative): the pairs (source, destination) of the live edges by id
    sg += "E";
    for (size_t e = 0; e < es.size(); e++) if (es[e] >= 0) { snprintf(buf, sizeof buf, " %d>%d", idx[es[e]], idx[ed[e]]); sg += buf; }
    return sg;
  }

  // ---- condensing (mbgraph.py:184-271, 479-498, 1315-1321)
  int condense(int e) {
    int s = es[e], d = ed[e], w = ew[e];
    int c = new_node(bases[s] + bases[d].substr(w));
    if (s != d) { cnt[c] = cnt[s] + cnt[d]; prev[c] = prev[s] + prev[d]; }
    else { cnt[c] = cnt[s]; prev[c] = prev[s]; }
    norm[c] = norm[s] + norm[d];
    if (norm[c] == 0) cc[c] = cc[s] + cc[d];
    else cc[c] = (cc[s] * norm[s] + cc[d] * norm[d]) / norm[c];
    if (s == d) {
      kill_edge(e);
      { std::vector<int> t = oute[s]; for (int x : t) { int ne = link(c, ed[x], ew[x]); ecc[ne] = ecc[x]; kill_edge(x); } }
      { std::vector<int> t = ine[s]; for (int x : t) { int ne = link(es[x], c, ew[x]); ecc[ne] = ecc[x]; kill_edge(x); } }
      cc[c] = cc[s] / 2.0;
      norm[c] = norm[s];
      nreads[c] = nreads[s];
      nreads[s].clear();
      kill_node(s);
      return c;
    }
    { std::vector<int> t = ine[s]; for (int x : t) { link(es[x], c, ew[x]); kill_edge(x); } }
    { std::vector<int> t = oute[d]; for (int x : t) { link(c, ed[x], ew[x]); kill_edge(x); } }
    int shift = (int)bases[s].size() - w;
    // P1: the source's reads sorted by (read, index), without repeats; then the destination's that are not among them (a sorted
    // vector + bisection: a tree node per read was most of bridge_all for the X-nodes of a highly expressed transcript)
    const double tcs0 = laps ? tnow() : 0.0;
    std::vector<RI> src;
    src.swap(nreads[s]);                                             // (the source's list is given up below anyway)
    sort_runs(src);
    // the source's reads without repeats, then the destination's that are not among them, in ONE vector of the final size (the
    // lists of a highly expressed transcript hold 10^5 reads: no second copy when the destination's part is appended)
    std::vector<RI> out;
    out.reserve(src.size() + nreads[d].size());
    for (size_t q = 0; q < src.size(); q++) if (q == 0 || !(src[q] == src[q - 1])) out.push_back(src[q]);
    const size_t n_src = out.size();
    if (std::is_sorted(nreads[d].begin(), nreads[d].end())) {
      // (both lists ascending -- the shift keeps the order: one pass with a cursor into the source's part instead of a bisection per read)
      size_t a = 0;
      for (const RI& x : nreads[d]) {
        const RI y(x.first, x.second - shift);
        while (a < n_src && out[a] < y) a++;
        if (!(a < n_src && out[a] == y)) out.push_back(y);
      }
    } else
      for (const RI& x : nreads[d]) { RI y(x.first, x.second - shift); if (!std::binary_search(out.begin(), out.begin() + (ptrdiff_t)n_src, y)) out.push_back(y); }
    nreads[c].swap(out);
    if (laps) { t_cond_sort += tnow() - tcs0; v_cond += nreads[c].size(); }
    nreads[s].clear(); nreads[d].clear();
    kill_edge(e);
    kill_node(s); kill_node(d);
    return c;
  }
  void local_condense_edge(int e) {
    if (es[e] < 0) return;
    if (oute[es[e]].size() > 1 || ine[ed[e]].size() > 1) return;
    int c = condense(e);
    std::vector<int> t = ine[c];
    t.insert(t.end(), oute[c].begin(), oute[c].end());
    for (int x : t) local_condense_edge(x);
  }
  void local_condense_node(int n) {
    if (oute[n].size() == 1) local_condense_edge(oute[n][0]);
    if (ine[n].size() == 1) local_condense_edge(ine[n][0]);
  }
  void condense_all() {
    size_t i = 0;
    while (i < order.size()) {
      int n = order[i++];
      if (oute[n].size() != 1) continue;
      int e = oute[n][0], d = ed[e];
      if (ine[d].size() == 1 && n != d) condense(e);
    }
    remove_destroyed();
  }

  // ---- error pruning (mbgraph.py:1169-1313)
  bool is_suspicious(int n) const {
    size_t ni = ine[n].size(), no = oute[n].size();
    if ((int)bases[n].size() <= SIZE_THRESHOLD && (ni == 0 || no == 0)) return true;
    if (avg_prev(n) >= 1) return false;
    if (ni == 0 || no == 0) return true;
    { double t = 0; for (int e : ine[n]) t += (double)oute[es[e]].size(); if (t / (double)ni < 2) return false; }
    { double t = 0; for (int e : oute[n]) t += (double)ine[ed[e]].size(); if (t / (double)no < 2) return false; }
    return true;
  }
  void destroy_suspicious() {
    while (true) {
      std::vector<int> sus;
      for (int n : order) if (is_suspicious(n)) sus.push_back(n);
      if (sus.empty()) return;
      std::stable_sort(sus.begin(), sus.end(), [&](int a, int b) { return avg_prev(a) < avg_prev(b); });
      for (int n : sus) {
        if (dead[n]) continue;
        std::vector<int> adj = pred(n), s2 = succ(n);
        adj.insert(adj.end(), s2.begin(), s2.end());
        full_destroy(n);
        for (int a : adj) local_condense_node(a);
      }
      remove_destroyed();
    }
  }
  bool similar(int a, int b) const {
    if (dead[a] || dead[b]) return false;
    const std::string &x = bases[a], &y = bases[b];
    if (x.size() != y.size()) return false;
    size_t mism = 0;
    for (size_t i = 0; i < x.size(); i++) mism += x[i] != y[i];
    if ((double)mism / (double)std::max<size_t>(x.size(), 1) >= 0.1) return false;
    auto uniq = [](std::vector<int> v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); return v; };
    return uniq(succ(a)) == uniq(succ(b)) && uniq(pred(a)) == uniq(pred(b));
  }
  void collapse_all() {
    while (true) {
      bool collapsed = false;
      for (size_t oi = 0; oi < order.size(); oi++) {
        int n = order[oi];
        std::vector<int> ss;
        for (int s : succ(n)) if (!dead[s]) ss.push_back(s);
        bool done = false;
        for (size_t i = 0; i < ss.size() && !done; i++)
          for (size_t j = i + 1; j < ss.size(); j++)
            if (similar(ss[i], ss[j])) {
              int a = ss[i], b = ss[j];
              if (prev[a] < prev[b]) std::swap(a, b);
              prev[a] += prev[b];
              full_destroy(b);
              collapsed = done = true;
              break;
            }
      }
      remove_destroyed();
      if (!collapsed) return;
    }
  }

  // ---- bridging (mbgraph.py:77-111, 450-628)
  // a hit of the device's seed scan (the read holds the node's first K-mer at `index`, bit for bit): for a node that IS one K-mer --
  // nearly every X-node -- the text is matched already and what is left of read_bridges is its bounds, without a look at the read
  bool hit_bridges(int r, int n, int index) const {
    if ((int)bases[n].size() == K) return index > 0 && (int)reads.len(r) > index + K;
    return read_bridges(r, n, index);
  }
  bool read_bridges(int r, int n, int index) const {
    const RStr rb = reads.rstr(r); const std::string& nb = bases[n];
    if (index <= 0 || (int)rb.size() <= index + (int)nb.size()) return false;
    return rb.compare(index, nb.size(), nb) == 0;
  }
  // packed key of s[pos..pos+K) or false if it holds a non-ACGT character
  template <class S> bool key_at(const S& s, size_t pos, uint64_t& key) const {
    key = 0;
    for (int j = 0; j < K; j++) { int c = base_code(s[pos + j]); if (c < 0) return false; key = (key << 2) | (uint64_t)c; }
    return true;
  }
  // device copy of the distinct reads + pattern table; returns false if the GPU path is not usable
  // the distinct reads on the device: rows of the resident input (device gather; 5 bytes per read cross the bus), else their text
  bool ensure_dreads(shn_reads** dreads) {
    if (!ctx || reads.n_rd() == 0 || !reads.text_all_acgt()) return false;
    if (*dreads) return true;
    if (reads.src_a && reads.dd && reads.dd->n_distinct == reads.n_rd()) return shn_reads_gather_dev(ctx, reads.src_a, reads.src_b, reads.dd->d_row, reads.dd->d_flag, reads.n_rd(), dreads) == 0;
    if (reads.src_a && reads.origin_row.size() == reads.n_rd()) return shn_reads_gather(ctx, reads.src_a, reads.src_b, reads.origin_row.data(), reads.origin_flag.data(), reads.n_rd(), dreads) == 0;
    return shn_reads_create(ctx, (const uint8_t*)reads.rindex.arena.data(), reads.rindex.off.data(), reads.n_rd(), 0, SHN_ENC_ASCII, dreads) == 0;
  }
  bool gpu_patterns(const SeedIndex& si, shn_reads** dreads, shn_table** tab) {
    if (!ctx || K > 32 || reads.n_rd() == 0 || si.keys.empty() || !reads.text_all_acgt()) return false;
    if (!ensure_dreads(dreads)) return false;
    std::vector<uint32_t> vals(si.keys.size());
    for (size_t i = 0; i < vals.size(); i++) vals[i] = (uint32_t)i + 1;
    return shn_table_create(ctx, si.keys.data(), vals.data(), si.keys.size(), K, 0, tab) == 0;
  }
  shn_reads* d_reads = nullptr;
  void release_gpu() { if (d_reads) { shn_reads_destroy(d_reads); d_reads = nullptr; } }

  void find_bridging_reads() {
    std::vector<std::pair<uint64_t, std::pair<int, int>>> items;
    for (int n : order) if (is_xnode(n)) { uint64_t key; if (key_at(bases[n], 0, key)) items.push_back({key, {n, 0}}); }
    if (items.empty()) return;
    SeedIndex si;
    si.build(items);
    shn_table* tab = nullptr;
    {
      // GPU section (on this thread's own context / stream)
      bool gpu_ok = false;
      uint64_t nh = 0;
      std::vector<uint32_t> hr, hs, hi;
      {
        const double tf0 = laps ? tnow() : 0.0;
        double tf1 = tf0, tf2 = tf0;
        if (gpu_patterns(si, &d_reads, &tab)) {
          if (laps) tf1 = tnow();
          gpu_ok = shn_seed_scan(ctx, d_reads, K, tab, &nh, nullptr, nullptr, nullptr) == 0;
          if (laps) tf2 = tnow();
          if (gpu_ok && nh) {
            hr.resize(nh); hs.resize(nh); hi.resize(nh);
            gpu_ok = shn_seed_scan(ctx, d_reads, K, tab, &nh, hr.data(), hs.data(), hi.data()) == 0;
          }
          shn_table_destroy(tab);
        }
        if (laps) fprintf(stderr, "[mbgraph]   find_bridging_reads: reads + patterns on the device %.3f s, count pass %.3f s, fill pass + download %.3f s (%llu hits, %zu patterns)\n",
                          tf1 - tf0, tf2 - tf1, tnow() - tf2, (unsigned long long)nh, si.keys.size());
      }
      if (gpu_ok) {
        // the hits against the node texts (read_bridges: the read spells the whole node with a base to spare on either side) -- on the
        // host threads that are free right now when there are many (the largest partition of BASELINE configs[2]: 415 k hits, 30-58 ms
        // on one thread, with the other partitions long done): slices of the hit list in order, each thread's confirmed hits kept in
        // order and appended slice by slice, so every node's list is what the one-thread loop makes
        const unsigned want = nh >= 100000 ? (unsigned)std::min<uint64_t>(8, nh / 50000) : 1u;
        const FreeThreads free_threads(want);
        const unsigned nt = free_threads.n;
        if (nt > 1) {
          std::vector<std::vector<std::pair<int, RI>>> found(nt);
          run_on_threads(nt, [&](unsigned t) {
            std::vector<std::pair<int, RI>>& out = found[t];
            const uint64_t h0 = nh * t / nt, h1 = nh * (t + 1) / nt;
            for (uint64_t h = h0; h < h1; h++) {
              if (h + 12 < h1) reads.prefetch_read((int)hr[h + 12]);
              for (uint32_t q = si.goff[hi[h]]; q < si.goff[hi[h] + 1]; q++) {
                const int x = si.occ[q].first;
                if (hit_bridges((int)hr[h], x, (int)hs[h])) out.push_back({x, RI((int)hr[h], (int)hs[h])});
              }
            }
          });
          for (unsigned t = 0; t < nt; t++) for (const auto& xr : found[t]) nreads[xr.first].push_back(xr.second);
          return;
        }
        for (uint64_t h = 0; h < nh; h++) {
          if (h + 12 < nh) reads.prefetch_read((int)hr[h + 12]);
          for (uint32_t q = si.goff[hi[h]]; q < si.goff[hi[h] + 1]; q++) {
            int x = si.occ[q].first;
            if (hit_bridges((int)hr[h], x, (int)hs[h])) nreads[x].push_back(RI((int)hr[h], (int)hs[h]));
          }
        }
        return;
      }
    }
    const uint64_t mask = K == 32 ? ~0ULL : ((1ULL << (2 * K)) - 1);
    for (int r = 0; r < (int)reads.n_rd(); r++) {
      const RStr rb = reads.rstr(r);
      uint64_t key = 0;
      int valid = 0;
      for (int i = 0; i < (int)rb.size(); i++) {
        int c = base_code(rb[i]);
        if (c < 0) { valid = 0; key = 0; continue; }
        key = ((key << 2) | (uint64_t)c) & mask;
        if (++valid < K) continue;
        int s0 = i - K + 1;                                  // window start; the reference scans range(1, len-K)
        if (s0 < 1 || s0 >= (int)rb.size() - K) continue;
        int gi = si.find(key);
        if (gi < 0) continue;
        for (uint32_t q = si.goff[gi]; q < si.goff[gi + 1]; q++) {
          int x = si.occ[q].first;
          if (read_bridges(r, x, s0)) nreads[x].push_back(RI(r, s0));
        }
      }
    }
  }
  void refresh_bridging_reads(int n) {
    const double tr0 = laps ? tnow() : 0.0;
    struct Lap { Graph* g; double t0; size_t v; ~Lap() { if (g->laps) { g->t_refresh += tnow() - t0; g->n_refresh++; g->v_refresh += v; } } } lap_{this, tr0, nreads[n].size()};
    const std::string& nb = bases[n];
    int lb = (int)nb.size();
    // (the reference collects them in a set and the pinned order P1 walks it sorted: a sorted vector without repeats is the same
    // sequence -- the lists of a highly expressed X-node hold 10^5 reads, and a tree insert per read was most of bridge_all)
    // the characters the neighbours put in front of / behind the node (the same for every read of the list)
    bool in_ch[256] = {false}, out_ch[256] = {false};
    if (!nreads[n].empty()) {
      for (int e : ine[n]) { const std::string& pb = bases[es[e]]; in_ch[(unsigned char)pb[pb.size() - ew[e] - 1]] = true; }
      for (int e : oute[n]) out_ch[(unsigned char)bases[ed[e]][ew[e]]] = true;
    }
    // one pass over the list: the read spells the node from i on, and the characters before and behind are ones a neighbour offers
    // (the reference filters by text, orders, then filters by the neighbours: the filters commute, the order comes last here)
    std::vector<RI> rs;
    rs.reserve(nreads[n].size());
    const std::vector<RI>& in_list = nreads[n];
    for (size_t q = 0; q < in_list.size(); q++) {
      if (q + 8 < in_list.size()) reads.prefetch_read(in_list[q + 8].first);
      const RI& x = in_list[q];
      const int r = x.first, i = x.second;
      if (i <= 0) continue;
      const RStr rb = reads.rstr(r);
      if ((int)rb.size() > i + lb && in_ch[(unsigned char)rb[i - 1]] && out_ch[(unsigned char)rb[i + lb]] && rb.compare(i, lb, nb) == 0) rs.push_back(x);
    }
    sort_runs(rs);
    rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
    nreads[n].swap(rs);
  }
  // bridge_all asks every X-node in every pass; the answer depends on the node's edge lists (edge ids: an edge never changes its
  // ends or its weight), on its bridging reads (which only this function filters, idempotently, between two passes -- bridging
  // appends reads to the NEW nodes it makes) and on texts that never change: an X-node whose edge lists and read count are what
  // they were at the last call gets the last answer, without going through its 10^3-10^5 reads again
  struct BridgedMemo { std::vector<int> in, out; size_t n_reads = (size_t)-1; bool answer = false; };
  std::vector<BridgedMemo> bridged_memo;
  bool is_bridged_xnode(int n) {
    if (bridged_memo.size() < bases.size()) bridged_memo.resize(bases.size());
    BridgedMemo& memo = bridged_memo[n];
    if (memo.n_reads == nreads[n].size() && memo.in == ine[n] && memo.out == oute[n]) return memo.answer;
    const bool ans = is_bridged_xnode_now(n);
    BridgedMemo& m2 = bridged_memo[n];
    m2.in = ine[n]; m2.out = oute[n]; m2.n_reads = nreads[n].size(); m2.answer = ans;
    return ans;
  }
  bool is_bridged_xnode_now(int n) {
    refresh_bridging_reads(n);
    int lb = (int)bases[n].size();
    bool inb[256] = {false}, outb[256] = {false};                  // (the distinct characters before / behind the node in its reads)
    int n_in = 0, n_out = 0;
    for (const RI& x : nreads[n]) {
      const RStr rb = reads.rstr(x.first);
      const unsigned char a = (unsigned char)rb[x.second - 1], b = (unsigned char)rb[x.second + lb];
      if (!inb[a]) { inb[a] = true; n_in++; }
      if (!outb[b]) { outb[b] = true; n_out++; }
    }
    int bi = (int)ine[n].size() - n_in, bo = (int)oute[n].size() - n_out;
    return (bi == 0 && bo == 0) || (bi == 1 && bo == 1);
  }
  int bridging_step(int node) {
    // (bridge_all has just asked is_bridged_xnode about this node: unless a bridging step in between touched its edges, its reads
    // are filtered already)
    if (!((size_t)node < bridged_memo.size() && bridged_memo[node].n_reads == nreads[node].size() && bridged_memo[node].in == ine[node] &&
          bridged_memo[node].out == oute[node]))
      refresh_bridging_reads(node);
    if (nreads[node].empty() || ine[node].size() < 2 || oute[node].size() < 2) return shn_fail(SHN_ERR_INTERNAL, "bridging_step: assertion failed");
    const std::string nb = bases[node];
    int lb = (int)nb.size();
    std::vector<int> u_list, w_list;
    int v_back = -1, v_forward = -1, loop_w = 0;
    double tb0 = laps ? tnow() : 0.0;
    if (laps) { n_steps++; v_bs += nreads[node].size(); }
    { std::vector<int> t = ine[node];
      for (int e : t) {
        int p = es[e], w = ew[e];
        const std::string& pb = bases[p];
        const char cp = pb[pb.size() - w - 1];
        int u = new_node(std::string(1, cp) + nb);
        link(p, u, w + 1);
        bridged[u] = 0;
        if (p == node) { v_back = u; loop_w = w; }
        u_list.push_back(u);
      }
      // read_bridges(read, u, i - 1) for a read the refresh above left in the list (i > 0, the read longer than i + lb, its text equal
      // to the node's from i on): the read reaches one base further back and that base is u's first -- no text to compare again.
      // One pass over the reads for all the u-nodes (each gets the reads with its character, in list order).
      const std::vector<RI>& lst = nreads[node];
      for (size_t q = 0; q < lst.size(); q++) {
        if (q + 8 < lst.size()) reads.prefetch_read(lst[q + 8].first);
        const RI& x = lst[q];
        if (x.second - 1 <= 0) continue;
        const char c = reads.rstr(x.first)[x.second - 1];
        for (int u : u_list) if (bases[u][0] == c) nreads[u].push_back(RI(x.first, x.second - 1));
      } }
    if (laps) { const double t = tnow(); t_bs_in += t - tb0; tb0 = t; }
    { std::vector<int> t = oute[node];
      for (int e : t) {
        int q = ed[e], w = ew[e];
        int x = new_node(nb + std::string(1, bases[q][w]));
        link(x, q, w + 1);
        for (const RI& y : nreads[node]) if (read_bridges(y.first, x, y.second + 1)) nreads[x].push_back(RI(y.first, y.second + 1));
        bridged[x] = 0;
        if (q == node) v_forward = x;
        w_list.push_back(x);
      } }
    if (laps) { const double t = tnow(); t_bs_out += t - tb0; tb0 = t; }
    { std::vector<int> t = ine[node]; for (int e : t) kill_edge(e); }
    { std::vector<int> t = oute[node]; for (int e : t) kill_edge(e); }
    if (v_back >= 0) {
      if (v_forward < 0) return shn_fail(SHN_ERR_INTERNAL, "bridging_step: self loop without forward node");
      link(v_forward, v_back, loop_w + 2);
    }
    std::map<int, int> links;
    for (int n : u_list) links[n] = 0;
    for (int n : w_list) links[n] = 0;
    std::vector<RI> rl = nreads[node];
    // (the u-nodes are `base + node text`, the w-nodes `node text + base` -- all lb + 1 bases long --, and the read equals the node
    // text from i on: one base decides; the bases looked up once, not per read)
    std::vector<char> u_ch(u_list.size()), w_ch(w_list.size());
    for (size_t a = 0; a < u_list.size(); a++) u_ch[a] = (int)bases[u_list[a]].size() == lb + 1 ? bases[u_list[a]][0] : '\0';
    for (size_t a = 0; a < w_list.size(); a++) w_ch[a] = (int)bases[w_list[a]].size() == lb + 1 ? bases[w_list[a]][lb] : '\0';
    for (size_t q = 0; q < rl.size(); q++) {
      if (q + 8 < rl.size()) reads.prefetch_read(rl[q + 8].first);
      const RI& y = rl[q];
      const RStr rb = reads.rstr(y.first);
      int i = y.second;
      // exactly one u-node spelling the read from i - 1 and one w-node spelling it from i
      int u = -1, x = -1, nu = 0, nw = 0;
      if (rb.size() >= (size_t)(i + lb)) { const char c = rb[i - 1]; for (size_t a = 0; a < u_ch.size(); a++) if (u_ch[a] == c && c) { u = u_list[a]; nu++; } }
      if (rb.size() >= (size_t)(i + lb + 1)) { const char c = rb[i + lb]; for (size_t a = 0; a < w_ch.size(); a++) if (w_ch[a] == c && c) { x = w_list[a]; nw++; } }
      if (nu != 1 || nw != 1) continue;
      nreads[u].push_back(RI(y.first, i - 1));
      nreads[x].push_back(RI(y.first, i));
      bool prec = false;
      for (int e : oute[u]) if (ed[e] == x) prec = true;
      if (!prec) { link(u, x, lb); bridged[u] = 1; bridged[x] = 1; links[u]++; links[x]++; }
    }
    nreads[node].clear();
    if (laps) { const double t = tnow(); t_bs_rl += t - tb0; tb0 = t; }
    std::vector<int> ub_u, ub_w;
    for (int u : u_list) if (bridged[u] != 1) ub_u.push_back(u);
    for (int x : w_list) if (bridged[x] != 1) ub_w.push_back(x);
    if (ub_u.size() == 1 && ub_w.size() == 1) { link(ub_u[0], ub_w[0], lb); links[ub_u[0]]++; links[ub_w[0]]++; }
    else if (ub_u.size() + ub_w.size() != 0) return shn_fail(SHN_ERR_INTERNAL, "bridging_step: unbridged edges remain");
    int link_count = 0;
    for (auto& kv : links) link_count += kv.second;
    std::vector<int> all = u_list;
    all.insert(all.end(), w_list.begin(), w_list.end());
    for (int n : all) prev[n] = ((double)links[n] / (double)link_count) * prev[node];
    const double tc0 = laps ? tnow() : 0.0;
    for (int n : all) {
      std::vector<int> t = ine[n];
      t.insert(t.end(), oute[n].begin(), oute[n].end());
      for (int e : t) local_condense_edge(e);
    }
    if (laps) t_condense += tnow() - tc0;
    kill_node(node);
    return 0;
  }
  double t_condense = 0, t_refresh = 0, t_bs_in = 0, t_bs_out = 0, t_bs_rl = 0, t_cond_sort = 0;
  size_t n_refresh = 0, v_refresh = 0, v_bs = 0, v_cond = 0, n_steps = 0;
  int bridge_all() {
    double t_ask = 0, t_step = 0;
    size_t n_ask = 0;
    while (true) {
      std::vector<int> todo;
      double t0 = tnow();
      {
        // the X-nodes whose last answer does not stand any more: each one's question touches its own read list and memo only (and
        // read text, see decode_lazy), so they are asked on the host threads that are free right now -- late in the stage, when the
        // largest partition is at its bridging alone, that is most of them
        std::vector<int> stale;
        if (bridged_memo.size() < bases.size()) bridged_memo.resize(bases.size());
        for (int n : order) if (is_xnode(n)) {
          const BridgedMemo& memo = bridged_memo[n];
          if (!(memo.n_reads == nreads[n].size() && memo.in == ine[n] && memo.out == oute[n])) stale.push_back(n);
        }
        size_t work = 0;
        for (int n : stale) work += nreads[n].size();
        const unsigned want = work >= 50000 && stale.size() >= 8 ? (unsigned)std::min<size_t>(8, stale.size() / 4) : 1u;
        const FreeThreads free_threads(want);
        if (free_threads.n > 1) {
          std::atomic<size_t> next{0};
          run_on_threads(free_threads.n, [&](unsigned) { for (size_t i; (i = next.fetch_add(1)) < stale.size();) (void)is_bridged_xnode(stale[i]); });
        }
      }
      for (int n : order) if (is_xnode(n)) { n_ask++; if (is_bridged_xnode(n)) todo.push_back(n); }
      double t1 = tnow();
      for (int n : todo) { int rc = bridging_step(n); if (rc) return rc; }
      t_ask += t1 - t0; t_step += tnow() - t1;
      bridged_log.push_back((int)todo.size());
      remove_destroyed();
      if (todo.empty()) {
        if (laps) fprintf(stderr, "[mbgraph]   bridge_all: %zu passes, is_bridged_xnode %.3f s (%zu questions), bridging_step %.3f s (%.3f s of it condensing)\n",
                          bridged_log.size(), t_ask, n_ask, t_step, t_condense);
        if (laps) fprintf(stderr, "[mbgraph]   bridge_all: refresh %.3f s (%zu calls, %zu reads), steps %zu (%zu reads): in %.3f out %.3f distribute %.3f s; condense read lists %.3f s (%zu reads)\n",
                          t_refresh, n_refresh, v_refresh, n_steps, v_bs, t_bs_in, t_bs_out, t_bs_rl, t_cond_sort, v_cond);
        return 0;
      }
    }
  }

  // ---- copy counts, cycles (mbgraph.py:735-767, 903-960, 1040-1049, 1133-1161, 1324-1331)
  void find_approximate_copy_counts() {
    known_paths.clear();
    for (int n : order) { norm[n] = (double)((int)bases[n].size() - K + 1); cc[n] = prev[n] / norm[n]; cc_int[n] = 0; }
    for (int n : order)
      for (int e : oute[n]) {
        int nm = std::max(L - ew[e] - 1, 0);
        int a = es[e], b = ed[e];
        double tot = cc[a] * norm[a] + cc[b] * norm[b];
        ecc[e] = nm == 0 ? 0.0 : 0.5 * tot / (double)nm;
      }
  }
  void disregard_loops() {
    for (int n : order) { bool self = false; for (int e : oute[n]) if (ed[e] == n) self = true; if (self) { norm[n] = 0; cc[n] = 0; } }
  }
  bool reachable_cycle(int n, std::set<int>& no_cycles, std::vector<int>& trav, std::vector<int>& out) {
    trav.push_back(n);
    std::vector<int> ss = succ(n);
    for (int m : ss) {
      auto it = std::find(trav.begin(), trav.end(), m);
      if (it != trav.end()) { out.assign(it, trav.end()); out.push_back(m); trav.pop_back(); return true; }
      if (no_cycles.count(m)) continue;
      if (reachable_cycle(m, no_cycles, trav, out)) { trav.pop_back(); return true; }
    }
    no_cycles.insert(n);
    trav.pop_back();
    return false;
  }
  bool find_cycle(std::set<int>& no_cycles, std::vector<int>& out) {
    for (int n : order) {
      if (no_cycles.count(n)) continue;
      std::vector<int> trav;
      if (reachable_cycle(n, no_cycles, trav, out)) return true;
    }
    return false;
  }
  int break_cycles() {
    std::set<int> no_cycles;
    std::vector<int> c;
    while (find_cycle(no_cycles, c)) full_destroy(c[1]);
    remove_destroyed();
    condense_all();
    std::set<int> chk;
    if (find_cycle(chk, c)) return shn_fail(SHN_ERR_INTERNAL, "break_cycles: graph still cyclic");
    return 0;
  }

  // ---- reads on the graph (mbgraph.py:1355-1441, 114-160, 839-880)
  template <class S> static bool compare(const S& a, size_t ao, const std::string& b, size_t bo) {
    size_t n = std::min(a.size() - ao, b.size() - bo);
    return memcmp(&a[0] + ao, b.data() + bo, n) == 0;
  }
  template <class S> void search_sequence(const S& seq, size_t so, int node, int i, int hops, std::vector<int>& cur, std::vector<std::vector<int>>& out) {
    size_t nl = bases[node].size() - i;
    cur.push_back(node);
    if (hops <= 0 || seq.size() - so <= nl) { out.push_back(cur); cur.pop_back(); return; }
    size_t so2 = so + nl;
    for (int e : oute[node])
      if (compare(seq, so2, bases[ed[e]], ew[e])) search_sequence(seq, so2, ed[e], ew[e], hops - 1, cur, out);
    cur.pop_back();
  }
  void find_known_paths() {
    known_paths.clear();
    double tk0 = tnow(), tk1 = 0, tk2 = 0, tk3 = 0;
    const uint64_t mask = K == 32 ? ~0ULL : ((1ULL << (2 * K)) - 1);
    // ---- device path (kpaths_gpu.hip): every read is classified where the reads are; the host searches only the reads that run
    // past the end of the node they start in, against an index of just their first K-mers
    {
      if (ctx && K <= 31 && shn_env_flag("SHN_GRAPH_KP_GPU", true) && reads.n_rd() && ensure_dreads(&d_reads)) {
        std::string nb;
        std::vector<uint64_t> noff(1, 0);
        { size_t tot = 0; for (int n : order) tot += bases[n].size(); nb.reserve(tot); noff.reserve(order.size() + 1); }
        for (int n : order) { nb += bases[n]; noff.push_back(nb.size()); }
        std::vector<uint8_t> st(reads.n_rd());
        std::vector<int32_t> nd(reads.n_rd());
        std::vector<uint32_t> no(reads.n_rd());
        // the out-edges of the nodes in list order, for the device's search of the reads that run past their first node (kp_search):
        // destination as an index into `order`, and the offset into the destination at which it continues the source
        std::vector<uint32_t> eoff(order.size() + 1, 0), edst, eov;
        {
          std::unordered_map<int, uint32_t> pos_of;
          pos_of.reserve(order.size() * 2);
          for (size_t q = 0; q < order.size(); q++) pos_of[order[q]] = (uint32_t)q;
          for (size_t q = 0; q < order.size(); q++) {
            for (int e : oute[order[q]]) { edst.push_back(pos_of[ed[e]]); eov.push_back((uint32_t)ew[e]); }
            eoff[q + 1] = (uint32_t)edst.size();
          }
        }
        // room for the records [read, length, nodes ...] of the searched reads: a few words per read that runs on (4 % of the reads do)
        std::vector<int32_t> precs(std::max<size_t>(1u << 16, reads.n_rd() / 2 + 4096));
        uint64_t precs_used = 0;
        tk1 = tnow();
        if (reads.dev_attrs) {
          // everything per read stays on the device: the host gets the reads left to search, the records of the reads searched
          // there and (below, after its own searches) the node pairs of find_mate_pairs
          std::vector<KpSlow> left;
          std::vector<int32_t> recs;
          std::vector<uint32_t> rec_cnt;
          if (kp) { shn_kp_destroy(kp); kp = nullptr; }
          const int rcf = shn_known_paths_dev(ctx, d_reads, K, (const uint8_t*)nb.data(), noff.data(), order.size(), eoff.data(), edst.data(), eov.data(), reads.dd, &left,
                                              &recs, &rec_cnt, &kp);
          release_gpu();
          tk2 = tnow();
          if (rcf == 0) {
            std::unordered_map<int, int> pos_in_order;
            FlatSum cnt_of(rec_cnt.size() / 2 + 16);                 // (a searched read's copies: every read has one entry)
            for (size_t i = 0; i + 1 < rec_cnt.size(); i += 2) cnt_of.set(rec_cnt[i], (double)rec_cnt[i + 1]);
            int cntp = 0;
            FlatSum edge_sum(4096);
            std::unordered_map<uint64_t, std::vector<std::vector<int>>> seen;
            auto add_path = [&](const std::vector<int>& pth, double copies) {
              for (size_t j = 0; j + 1 < pth.size(); j++) edge_sum.add(((uint64_t)(uint32_t)pth[j] << 32) | (uint32_t)pth[j + 1], copies);
              if (pth.size() > 2) {
                cntp++;
                uint64_t h = 0xcbf29ce484222325ULL;
                for (int v : pth) h = (h ^ (uint64_t)(uint32_t)v) * 0x100000001b3ULL;
                auto& lst = seen[h];
                bool have = false;
                for (const auto& q : lst) if (q == pth) { have = true; break; }
                if (!have) { lst.push_back(pth); known_paths.insert(pth); }
              }
            };
            std::vector<int> pth;
            for (uint64_t at = 0; at + 2 <= recs.size();) {
              const int32_t r = recs[at], len = recs[at + 1];
              if (len <= 0 || at + 2 + (uint64_t)len > recs.size()) break;
              pth.resize((size_t)len);
              for (int32_t j = 0; j < len; j++) pth[(size_t)j] = order[(size_t)recs[at + 2 + (uint64_t)j]];
              at += 2 + (uint64_t)len;
              add_path(pth, cnt_of.get((uint64_t)(uint32_t)r));
            }
            tk3 = tnow();
            // the reads the device left (a search deeper than its stack, no room for the records): the host's search, one by one
            std::vector<int32_t> patches;
            if (!left.empty()) {
              for (size_t q = 0; q < order.size(); q++) pos_in_order[order[q]] = (int)q;
              std::sort(left.begin(), left.end(), [](const KpSlow& a, const KpSlow& b) { return a.read < b.read; });
              // occurrences (node, offset), in index order, of the first K-mers of the reads of state 2
              std::unordered_map<uint64_t, std::vector<std::pair<int, int>>> occ_of;
              for (const KpSlow& sl : left) if (sl.state == 2) { uint64_t key; if (key_at(reads.rstr((int)sl.read), 0, key)) occ_of[key]; }
              if (!occ_of.empty())
                for (int n : order) {
                  const std::string& b = bases[n];
                  uint64_t key = 0;
                  for (int i = 0; i < (int)b.size(); i++) {
                    key = ((key << 2) | (uint64_t)base_code(b[i])) & mask;
                    if (i + 1 < K) continue;
                    auto it = occ_of.find(key);
                    if (it != occ_of.end()) it->second.push_back({n, i - K + 1});
                  }
                }
              std::vector<std::vector<int>> paths;
              std::vector<int> cur;
              std::vector<std::pair<int, int>> one(1);
              static const std::vector<std::pair<int, int>> none;
              for (const KpSlow& sl : left) {
                const int r = (int)sl.read;
                const RStr rb = reads.rstr(r);
                uint64_t key;
                if (!key_at(rb, 0, key)) continue;
                const std::vector<std::pair<int, int>>* occs = &one;
                if (sl.state == 3) one[0] = {order[sl.node], (int)sl.offset};
                else { auto it = occ_of.find(key); occs = it == occ_of.end() ? &none : &it->second; }
                int pf = -1, pl = -1;
                for (const auto& oc : *occs) {
                  const int sn = oc.first, so = oc.second;
                  if (!compare(rb, 0, bases[sn], so)) continue;
                  if (rb.size() <= bases[sn].size() - (size_t)so) { pf = sn; pl = sn; continue; }
                  paths.clear(); cur.clear();
                  search_sequence(rb, 0, sn, so, 30, cur, paths);
                  for (auto& p : paths) { pf = p.front(); pl = p.back(); add_path(p, (double)sl.cnt); }
                }
                patches.push_back(r); patches.push_back(pf < 0 ? -1 : pos_in_order[pf]); patches.push_back(pl < 0 ? -1 : pos_in_order[pl]);
              }
            }
            edge_sum.each([&](uint64_t k, double v) { known_edges[{(int)(uint32_t)(k >> 32), (int)(uint32_t)k}] += v; });
            n_known = cntp;
            // find_mate_pairs' pass over the reads, where their first / last nodes are (the graph does not change in between)
            mate_cand.clear();
            mate_cand_ready = shn_kp_mate_pairs(kp, reads.dd, patches.data(), patches.size() / 3, &mate_cand) == 0;
            if (mate_cand_ready) {
              for (uint32_t& x : mate_cand) x = (uint32_t)order[x];
              shn_kp_destroy(kp); kp = nullptr;
              if (laps) fprintf(stderr, "[mbgraph]   kp (device, resident) node text %.3f s scan + search %.3f s records %.3f s left to the host + mate pairs %.3f s  (%zu bases, %zu reads, %zu with records, %zu left, %zu node pairs)\n",
                                tk1 - tk0, tk2 - tk1, tk3 - tk2, tnow() - tk3, nb.size(), reads.n_rd(), rec_cnt.size() / 2, left.size(), mate_cand.size() / 2);
              return;
            }
            // (the pairs could not be made on the device: the host's pass needs first / last per read -- start over with host arrays)
            known_paths.clear(); known_edges.clear(); n_known = 0;
          }
          if (kp) { shn_kp_destroy(kp); kp = nullptr; }
          if ((attrs_rc = reads.need_host_attrs())) return;
          if (!ensure_dreads(&d_reads)) { attrs_rc = shn_fail(SHN_ERR_INTERNAL, "find_known_paths: the distinct reads could not be gathered again"); return; }
          tk1 = tnow();
        }
        const bool kp_dev_search = shn_env_flag("SHN_GRAPH_KP_SEARCH", true);
        const int rcs = kp_dev_search
            ? shn_known_paths_search(ctx, d_reads, K, (const uint8_t*)nb.data(), noff.data(), order.size(), eoff.data(), edst.data(), eov.data(), st.data(),
                                     nd.data(), no.data(), precs.data(), precs.size(), &precs_used)
            : shn_known_paths_scan(ctx, d_reads, K, (const uint8_t*)nb.data(), noff.data(), order.size(), st.data(), nd.data(), no.data());
        release_gpu();
        tk2 = tnow();
        if (rcs == 0) {
          // occurrences (node, offset), in index order, of the first K-mers of the reads left to search whose K-mer occurs more
          // than once (state 2: none in most partitions -- the K-mers of a de Bruijn graph are distinct until bridging copies nodes)
          std::unordered_map<uint64_t, std::vector<std::pair<int, int>>> occ_of;
          std::vector<uint64_t> bits(1u << 12, 0);                        // 2^18-bit filter in front of the map
          size_t n_slow = 0, n_multi = 0;
          {
            // the reads inside one node get that node as first / last (a pass over every read: on the threads that are free right now)
            const size_t nr = reads.n_rd();
            const unsigned want0 = (unsigned)std::max<size_t>(1, std::min<size_t>(8, nr >> 19));
            const FreeThreads free_threads(want0);
            const unsigned nt0 = free_threads.n;
            std::vector<size_t> slow_of(nt0, 0);
            std::vector<std::vector<uint32_t>> multi_of(nt0);
            run_on_threads(nt0, [&](unsigned t) {
              size_t ns = 0;
              for (size_t r = nr * t / nt0; r < nr * (t + 1) / nt0; r++) {
                const uint8_t v = st[r];
                if (v == 1) { const int n = order[nd[r]]; reads.rfirst[r] = n; reads.rlast[r] = n; reads.rhas[r] = 1; }
                else if (v == 3) ns++;
                else if (v == 2) { ns++; multi_of[t].push_back((uint32_t)r); }
              }
              slow_of[t] = ns;
            });
            for (unsigned t = 0; t < nt0; t++) {
              n_slow += slow_of[t];
              for (uint32_t r : multi_of[t]) {
                uint64_t key;
                n_multi++;
                if (key_at(reads.rstr((int)r), 0, key)) { occ_of[key]; const uint64_t h = fm_mix(key) >> 46; bits[h >> 6] |= 1ULL << (h & 63); }
              }
            }
          }
          if (n_multi)
            for (int n : order) {
              const std::string& b = bases[n];
              uint64_t key = 0;
              for (int i = 0; i < (int)b.size(); i++) {
                key = ((key << 2) | (uint64_t)base_code(b[i])) & mask;
                if (i + 1 < K) continue;
                const uint64_t h = fm_mix(key) >> 46;
                if (!((bits[h >> 6] >> (h & 63)) & 1)) continue;
                auto it = occ_of.find(key);
                if (it != occ_of.end()) it->second.push_back({n, i - K + 1});
              }
            }
          tk3 = tnow();
          // The reads left to search, on host threads (slices of whole 64-read words: the lazily decoded text keeps one done bit per
          // read).  Per thread: the sums per edge and the paths seen go through hash tables while the reads go by (10^5 reads of a highly
          // expressed transcript name the same few edges and paths) and are merged afterwards; the copy counts of reads are whole
          // numbers, so neither the order of the additions nor the cut into slices shows in the sums; a read's first / last node is its own.
          struct Local {
            FlatSum edge_sum;
            std::unordered_map<uint64_t, std::vector<std::vector<int>>> path_seen;
            std::vector<std::vector<int>> fresh;                           // distinct paths of this slice
            int cntp = 0;
          };
          auto search_slice = [&](size_t lo, size_t hi, Local& L) {
            std::vector<std::vector<int>> paths;
            std::vector<int> cur;
            std::vector<std::pair<int, int>> one(1);
            static const std::vector<std::pair<int, int>> none;
            for (size_t r = lo; r < hi; r++) {
              if (st[r] < 2 || st[r] == 4) continue;            // (4: searched on the device, its paths come in the records)
              const RStr rb = reads.rstr((int)r);
              uint64_t key;
              if (!key_at(rb, 0, key)) continue;
              const std::vector<std::pair<int, int>>* occs = &one;
              if (st[r] == 3) one[0] = {order[nd[r]], (int)no[r]};
              else { auto it = occ_of.find(key); occs = it == occ_of.end() ? &none : &it->second; }
              for (const auto& oc : *occs) {
                const int sn = oc.first, so = oc.second;
                if (!compare(rb, 0, bases[sn], so)) continue;
                if (rb.size() <= bases[sn].size() - (size_t)so) { reads.rfirst[r] = sn; reads.rlast[r] = sn; reads.rhas[r] = 1; continue; }
                paths.clear(); cur.clear();
                search_sequence(rb, 0, sn, so, 30, cur, paths);
                for (auto& p : paths) {
                  reads.rfirst[r] = p.front(); reads.rlast[r] = p.back(); reads.rhas[r] = 1;
                  for (size_t j = 0; j + 1 < p.size(); j++) L.edge_sum.add(((uint64_t)(uint32_t)p[j] << 32) | (uint32_t)p[j + 1], reads.rcc[r]);
                  if (p.size() > 2) {
                    L.cntp++;
                    uint64_t h = 0xcbf29ce484222325ULL;
                    for (int v : p) h = (h ^ (uint64_t)(uint32_t)v) * 0x100000001b3ULL;
                    auto& lst = L.path_seen[h];
                    bool have = false;
                    for (const auto& q : lst) if (q == p) { have = true; break; }
                    if (!have) { lst.push_back(p); L.fresh.push_back(p); }
                  }
                }
              }
            }
          };
          const unsigned want = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(16, std::max(1, shn_host_cpus())), n_slow >> 12));
          const FreeThreads free_threads(want);                              // (what is free right now: no waiting, no overdraft)
          const unsigned nts = free_threads.n;
          const size_t nr = reads.n_rd(), words = (nr + 63) / 64;
          std::vector<Local> locals(nts);
          run_on_threads(nts, [&](unsigned t) { search_slice(std::min(nr, words * t / nts * 64), std::min(nr, words * (t + 1) / nts * 64), locals[t]); });
          int cntp = 0;
          for (Local& L : locals) {
            cntp += L.cntp;
            L.edge_sum.each([&](uint64_t k, double v) { known_edges[{(int)(uint32_t)(k >> 32), (int)(uint32_t)k}] += v; });
            for (auto& p : L.fresh) known_paths.insert(std::move(p));
          }
          // the reads the device searched (state 4): their paths as it enumerated them, a read's records in the recursion's order (the
          // last one names its first / last node, mbgraph.py:1379-1384); the sums are of whole numbers, so no order shows in them
          {
            FlatSum edge_sum(4096);
            std::unordered_map<uint64_t, std::vector<std::vector<int>>> dev_seen;
            std::vector<int> pth;
            for (uint64_t at = 0; at + 2 <= precs_used;) {
              const int32_t r = precs[at], len = precs[at + 1];
              if (len <= 0 || at + 2 + (uint64_t)len > precs_used) break;
              pth.resize((size_t)len);
              for (int32_t j = 0; j < len; j++) pth[(size_t)j] = order[(size_t)precs[at + 2 + (uint64_t)j]];
              at += 2 + (uint64_t)len;
              reads.rfirst[r] = pth.front(); reads.rlast[r] = pth.back(); reads.rhas[r] = 1;
              for (size_t j = 0; j + 1 < pth.size(); j++) edge_sum.add(((uint64_t)(uint32_t)pth[j] << 32) | (uint32_t)pth[j + 1], reads.rcc[r]);
              if (pth.size() > 2) {
                cntp++;
                // (the 10^4-10^5 reads of a highly expressed transcript name the same few paths: a hash table in front of the ordered set)
                uint64_t h = 0xcbf29ce484222325ULL;
                for (int v : pth) h = (h ^ (uint64_t)(uint32_t)v) * 0x100000001b3ULL;
                auto& lst = dev_seen[h];
                bool have = false;
                for (const auto& q : lst) if (q == pth) { have = true; break; }
                if (!have) { lst.push_back(pth); known_paths.insert(pth); }
              }
            }
            edge_sum.each([&](uint64_t k, double v) { known_edges[{(int)(uint32_t)(k >> 32), (int)(uint32_t)k}] += v; });
          }
          n_known = cntp;
          if (laps) fprintf(stderr, "[mbgraph]   kp (device) node text %.3f s scan %.3f s slow index %.3f s search %.3f s  (%zu bases, %zu reads, %zu slow)\n", tk1 - tk0,
                            tk2 - tk1, tk3 - tk2, tnow() - tk3, nb.size(), reads.n_rd(), n_slow);
          return;
        }
      } }
    tk0 = tnow();
    if ((attrs_rc = reads.need_host_attrs())) return;          // (the host form works on per-read arrays of its own)
    reads.ensure_all_text();                                   // (the host form reads every read's text, on several threads)
    std::vector<std::pair<uint64_t, std::pair<int, int>>> items;
    for (int n : order) {
      const std::string& b = bases[n];
      uint64_t key = 0;
      int valid = 0;
      for (int i = 0; i < (int)b.size(); i++) {
        int c = base_code(b[i]);
        if (c < 0) { valid = 0; key = 0; continue; }
        key = ((key << 2) | (uint64_t)c) & mask;
        if (++valid >= K) items.push_back({key, {n, i - K + 1}});
      }
    }
    SeedIndex si;
    si.build(items);
    std::vector<uint32_t> first(reads.n_rd(), 0), last(reads.n_rd(), 0);     // group id + 1, 0 = absent
    shn_table* tab = nullptr;
    bool done = false;
    tk1 = tnow();
    {
      if (gpu_patterns(si, &d_reads, &tab)) {
        done = shn_seed_ends(ctx, d_reads, K, tab, first.data(), last.data()) == 0;
        shn_table_destroy(tab);
      }
    }
    if (!done)
      for (int r = 0; r < (int)reads.n_rd(); r++) {
        const RStr rb = reads.rstr(r);
        uint64_t key;
        if ((int)rb.size() < K) continue;
        if (key_at(rb, 0, key)) first[r] = (uint32_t)(si.find(key) + 1);
        if (key_at(rb, rb.size() - K, key)) last[r] = (uint32_t)(si.find(key) + 1);
      }
    release_gpu();
    tk2 = tnow();
    int cntp = 0;
    std::vector<std::vector<int>> paths;
    std::vector<int> cur;
    // Nearly every read lies inside one node: its only path is that node, it adds no known edge and no known path.  Those reads
    // are settled on host threads; the reads that cross node boundaries (`slow`) go through search_sequence one after the
    // other in read order, as the sums of known_edges require.
    std::vector<char> slow(reads.n_rd(), 0);
    {
      const unsigned ntp = (unsigned)std::min<size_t>(std::min<size_t>(16, std::max(1, shn_host_cpus() / 2)), std::max<size_t>(1, reads.n_rd() >> 18));
      auto classify = [&](size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; r++) {
          if (!first[r] || !last[r]) continue;
          const RStr rb = reads.rstr((int)r);
          const uint32_t gi = first[r] - 1;
          int fn = -1;
          bool any = false, need = false;
          for (uint32_t q = si.goff[gi]; q < si.goff[gi + 1] && !need; q++) {
            const int sn = si.occ[q].first, so = si.occ[q].second;
            if (!compare(rb, 0, bases[sn], so)) continue;
            if (rb.size() <= bases[sn].size() - (size_t)so) { fn = sn; any = true; }
            else need = true;
          }
          if (need) slow[r] = 1;
          else if (any) { reads.rfirst[r] = fn; reads.rlast[r] = fn; reads.rhas[r] = 1; }
        }
      };
      BudgetGuard budget((int)ntp);
      run_on_threads(ntp, reads.n_rd(), classify);
    }
    tk3 = tnow();
    size_t n_slow = 0;
    for (int r = 0; r < (int)reads.n_rd(); r++) {
      if (!slow[r]) continue;
      n_slow++;
      const RStr rb = reads.rstr(r);
      uint32_t gi = first[r] - 1;
      for (uint32_t q = si.goff[gi]; q < si.goff[gi + 1]; q++) {
        int sn = si.occ[q].first, so = si.occ[q].second;
        if (!compare(rb, 0, bases[sn], so)) continue;
        if (rb.size() <= bases[sn].size() - (size_t)so) {
          // the read lies inside this node (nearly all reads do): its only path is [sn] -- no edges, no known path
          reads.rfirst[r] = sn; reads.rlast[r] = sn; reads.rhas[r] = 1;
          continue;
        }
        paths.clear(); cur.clear();
        search_sequence(rb, 0, sn, so, 30, cur, paths);
        for (auto& p : paths) {
          reads.rfirst[r] = p.front(); reads.rlast[r] = p.back(); reads.rhas[r] = 1;
          for (size_t j = 0; j + 1 < p.size(); j++) known_edges[{p[j], p[j + 1]}] += reads.rcc[r];
          if (p.size() > 2) { known_paths.insert(p); cntp++; }
        }
      }
    }
    n_known = cntp;
    if (laps) fprintf(stderr, "[mbgraph]   kp index %.3f s gpu %.3f s classify %.3f s slow %.3f s  (%zu patterns, %zu reads, %zu slow)\n", tk1 - tk0, tk2 - tk1, tk3 - tk2,
                      tnow() - tk3, items.size(), reads.n_rd(), n_slow);
  }
  void find_copy_counts() {
    for (int n : order) {
      double tot = 0;
      bool any = false;
      for (int e : oute[n]) {
        auto it = known_edges.find({es[e], ed[e]});
        double ec = 0;
        if (it != known_edges.end()) { ec = it->second; any = true; }
        tot += ec;
        ecc[e] = ec / (double)std::max(L - ew[e] - 1, 1);
      }
      cc[n] = tot;
      cc_int[n] = any ? 0 : 1;      // Python: `tot` stays the int 0 when no out-edge has a known count
    }
  }
  void mate_search(int n, int goal, int max_len, int min_len, int hops, std::vector<int>& cur, std::vector<std::vector<int>>& out) {
    if (max_len <= 0 || hops <= 0) return;
    if (n == goal && min_len <= 1) { cur.push_back(goal); out.push_back(cur); cur.pop_back(); return; }
    cur.push_back(n);
    for (int e : oute[n]) {
      int nl = (int)bases[n].size() - ew[e];
      mate_search(ed[e], goal, max_len - nl, min_len - nl, hops - 1, cur, out);
    }
    cur.pop_back();
  }
  void find_mate_pairs() {
    std::vector<std::pair<int, int>> pairs;
    std::set<std::pair<int, int>> seen;
    if (reads.dev_attrs && mate_cand_ready) {
      // (made on the device right after the known-paths search, kpaths_gpu.hip: distinct (a, b), not adjacent, in no particular
      // order -- the loop below only counts and fills a set)
      for (size_t i = 0; i + 1 < mate_cand.size(); i += 2) if (seen.insert({(int)mate_cand[i], (int)mate_cand[i + 1]}).second) pairs.push_back({(int)mate_cand[i], (int)mate_cand[i + 1]});
    } else
    for (int r = 0; r < (int)reads.n_rd(); r++) {
      if (reads.rmp[r] != 1 || reads.rmate[r] < 0) continue;
      int m = reads.rmate[r];
      if (!reads.rhas[r] || !reads.rhas[m]) continue;
      int a = reads.rlast[r], b = reads.rfirst[m];
      if (a == b) continue;
      bool adj = false;
      for (int e : oute[a]) if (ed[e] == b) adj = true;
      if (adj) continue;
      if (seen.insert({a, b}).second) pairs.push_back({a, b});
    }
    int nmp = 0;
    for (auto& ab : pairs) {
      int a = ab.first, b = ab.second;
      const int fringe = 1, min_l = 0 - fringe, max_l = 300 - fringe;
      std::vector<std::vector<int>> paths;
      for (int e : oute[a]) {
        std::vector<int> cur(1, a);
        mate_search(ed[e], b, max_l + ew[e], min_l + ew[e], 7, cur, paths);
      }
      if (paths.size() == 1 && paths[0].size() > 2) { nmp++; known_paths.insert(paths[0]); }
    }
    n_mate = nmp;
  }

  int run() {
    double t0 = tnow();
    auto lap = [&](const char* what) { const double t = tnow(); lap_line(laps, what, t - t0, "nodes=%zu reads=%zu", order.size(), reads.n_rd()); t0 = t; };
    if (!precondensed) condense_all();
    nodes_after[0] = (int)order.size();
    lap("condense_all");
    destroy_suspicious();
    nodes_after[1] = (int)order.size();
    lap("destroy_suspicious");
    collapse_all();
    nodes_after[2] = (int)order.size();
    lap("collapse_all");
    find_bridging_reads();
    lap("find_bridging_reads");
    int rc = bridge_all();
    if (rc) return rc;
    lap("bridge_all");
    condense_all();
    nodes_after[3] = (int)order.size();
    find_approximate_copy_counts();
    disregard_loops();
    condense_all();
    remove_destroyed();
    lap("condense+copycounts");
    if ((rc = break_cycles())) return rc;
    lap("break_cycles");
    find_approximate_copy_counts();
    find_known_paths();
    if (attrs_rc) return attrs_rc;
    lap("find_known_paths");
    find_copy_counts();
    if (reads.dev_attrs && !mate_cand_ready && (rc = reads.need_host_attrs())) return rc;
    find_mate_pairs();
    lap("copy counts+mates");
    final_nodes = (int)order.size();
    return 0;
  }
};

}  // namespace

extern "C" void shn_graph_destroy(shn_graph* g) { delete g; }
int shn_graph_partitions_running() { return g_partitions_running.load(); }      // (sflow_host.hip: how many cores a sparse-flow call beside the graph stage may take)

// ---- what the entry points hand the driver: the partition's K-mer graph (KmerGraphSource) and its reads (ReadSource, mbgraph_reads.h)
// rows: n_rows k1-mers of K+1 bytes each (file order of component{c}k1mers_allowed.dict), and / or the partition's K-mer graph
// already contracted on the GPU (shn_unitigs_build, partition `part` of `ug`).  With ug the rows are needed when the partition holds
// a cycle of condensable edges (left to the sequential code) and for the development check SHN_GRAPH_CHECK=1 (both ways, compared).
struct KmerGraphSource { const uint8_t* rows = nullptr; uint64_t n_rows = 0; const shn_unitigs* ug = nullptr; uint32_t part = 0; };

// the graph before any read is looked at; n_kmer_nodes = its K-mers (the read cap is ten times that)
static int load_kmer_graph(Graph& g, const KmerGraphSource& ks, uint64_t& n_kmer_nodes) {
  const shn_unitigs* ug = ks.ug; const uint32_t part = ks.part;
  if (!ug || ug->cyclic[part]) {
    // (asked by the K-mers, not by the stored nodes: a partition that is nothing but cycles stores no node at all)
    if (ug && !ks.rows && ug->n_kmers[part] != 0) return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run_unitigs: cyclic partition needs the k1-mer rows");
    g.load_k1mers(ks.rows, ks.n_rows);
    n_kmer_nodes = g.order.size();
    return 0;
  }
  const uint64_t n0 = ug->node_off[part], n1 = ug->node_off[part + 1], e0 = ug->edge_off[part], e1 = ug->edge_off[part + 1];
  g.load_unitigs(ug->bases.data(), ug->base_off.data() + n0, ug->n_len.data() + n0, ug->n_tail_out.data() + n0, n1 - n0,
                 ug->e_src.data() + e0, ug->e_dst.data() + e0, ug->e_out_rank.data() + e0, ug->e_in_rank.data() + e0, e1 - e0);
  g.precondensed = true;
  n_kmer_nodes = ug->n_kmers[part];
  if (!shn_env_set("SHN_GRAPH_CHECK")) return 0;
  if (!ks.rows && ks.n_rows == 0 && n1 != n0) return shn_fail(SHN_ERR_ARG, "SHN_GRAPH_CHECK needs the k1-mer rows");
  Graph h;
  h.K = g.K;
  h.load_k1mers(ks.rows, ks.n_rows);
  const uint64_t hk = h.order.size();
  h.condense_all();
  if (hk == n_kmer_nodes && h.signature() == g.signature()) return 0;
  if (const char* dump = shn_env_str("SHN_GRAPH_CHECK_DUMP")) {
    FILE* fa = fopen((std::string(dump) + ".host").c_str(), "w"); if (fa) { fputs(h.signature().c_str(), fa); fclose(fa); }
    FILE* fb = fopen((std::string(dump) + ".gpu").c_str(), "w"); if (fb) { fputs(g.signature().c_str(), fb); fclose(fb); }
  }
  return shn_fail(SHN_ERR_INTERNAL, "SHN_GRAPH_CHECK: GPU unitigs differ from load_k1mers + condense_all (partition " + std::to_string(part) + ": " +
                  std::to_string(n_kmer_nodes) + " / " + std::to_string(hk) + " K-mers, " + std::to_string(g.order.size()) + " / " +
                  std::to_string(h.order.size()) + " nodes)");
}

// ---- output_components (add_component mbgraph.py:691-709, topological_sort :711-732, P2)
static shn_graph* export_components(Graph& g) {
  shn_graph* o = new shn_graph();
  o->s_off.push_back(0); o->n_off.push_back(0); o->p_off.push_back(0);
  o->comp_node_off.push_back(0); o->comp_edge_off.push_back(0); o->comp_path_off.push_back(0);
  std::map<int, std::vector<const std::vector<int>*>> by_start;
  for (auto& p : g.known_paths) by_start[p[0]].push_back(&p);
  for (int src : g.order) {
    if (g.dead[src]) continue;
    std::set<int> seen;
    std::set<int> edges;
    std::vector<int> queue(1, src);
    while (!queue.empty()) {
      int n = queue.back(); queue.pop_back();
      if (seen.count(n)) continue;
      seen.insert(n);
      for (int e : g.oute[n]) edges.insert(e);
      for (int e : g.oute[n]) queue.push_back(g.ed[e]);
      for (int e : g.ine[n]) queue.push_back(g.es[e]);
    }
    std::set<int> added;
    std::vector<int> topo, fringe;
    for (int n : seen) if (g.ine[n].empty()) fringe.push_back(n);      // `seen` iterates in creation (id) order
    while (!fringe.empty()) {
      int v = fringe.back(); fringe.pop_back();
      if (added.count(v)) continue;
      added.insert(v);
      topo.push_back(v);
      for (int e : g.oute[v]) {
        int n = g.ed[e];
        bool all = true;
        for (int pe : g.ine[n]) if (!added.count(g.es[pe])) all = false;
        if (all) fringe.push_back(n);
      }
    }
    if (topo.size() == 1) {
      g.hash[src] = -1;
      o->s_bases += g.bases[src];
      o->s_off.push_back(o->s_bases.size());
      o->s_cc.push_back(g.cc[src]); o->s_norm.push_back(g.norm[src]);
      g.dead[src] = 1;
      continue;
    }
    for (size_t h = 0; h < topo.size(); h++) { g.hash[topo[h]] = (int)h; g.dead[topo[h]] = 1; }
    for (int n : topo) {
      o->n_bases += g.bases[n];
      o->n_off.push_back(o->n_bases.size());
      o->n_cc.push_back(g.cc[n]); o->n_norm.push_back(g.norm[n]); o->n_cc_int.push_back((uint8_t)g.cc_int[n]);
    }
    o->comp_node_off.push_back(o->n_cc.size());
    for (int n : topo) {
      auto it = by_start.find(n);
      if (it == by_start.end()) continue;
      std::vector<std::vector<int>> ps;
      for (auto* p : it->second) { std::vector<int> h; for (int x : *p) h.push_back(g.hash[x]); ps.push_back(h); }
      std::sort(ps.begin(), ps.end());
      for (auto& h : ps) { for (int x : h) o->p_ids.push_back(x); o->p_off.push_back(o->p_ids.size()); }
    }
    o->comp_path_off.push_back(o->p_off.size() - 1);
    std::vector<std::array<double, 5>> el;
    for (int e : edges) if (g.ecc[e] > 0)
      el.push_back({(double)g.hash[g.es[e]], (double)g.hash[g.ed[e]], (double)g.ew[e], g.ecc[e], (double)std::max(g.L - g.ew[e] - 1, 0)});
    std::stable_sort(el.begin(), el.end(), [](const std::array<double, 5>& a, const std::array<double, 5>& b) {
      if (a[0] != b[0]) return a[0] < b[0];
      if (a[1] != b[1]) return a[1] < b[1];
      return a[2] < b[2];
    });
    for (auto& x : el) { o->e_in.push_back((int)x[0]); o->e_out.push_back((int)x[1]); o->e_w.push_back((int)x[2]); o->e_cc.push_back(x[3]); o->e_norm.push_back(x[4]); }
    o->comp_edge_off.push_back(o->e_in.size());
  }
  for (int i = 0; i < 4; i++) o->info.push_back(g.nodes_after[i]);
  o->info.push_back(g.final_nodes); o->info.push_back(g.n_known); o->info.push_back(g.n_mate);
  o->info.push_back((int)g.bridged_log.size());
  for (int b : g.bridged_log) o->info.push_back(b);
  return o;
}

// ---- the driver of one partition: every entry point below ends here
static int mbgraph_run(shn_ctx* ctx, int K, const KmerGraphSource& ks, ReadSource& rs, shn_graph** out) {
  if (!out || (ks.n_rows && !ks.rows) || (!rs.host_a && ((rs.n_reads && (!rs.r1 || !rs.r1_off)) || (rs.paired && rs.n_reads && (!rs.r2 || !rs.r2_off)))))
    return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run: NULL argument");
  struct Running { Running() { g_partitions_running.fetch_add(1); } ~Running() { g_partitions_running.fetch_sub(1); } } running;
  Graph g;
  g.ctx = shn_thread_ctx(ctx); g.K = K;
  g.L = rs.n_reads ? (int)rs.read_len() : -1;            // Read.L = length of the first read
  g.SIZE_THRESHOLD = g.L;
  // SHN_DEBUG: the laps of every partition; SHN_GRAPH_LAPS=n: of the partitions with at least n routed reads
  g.laps = g.reads.laps = shn_env_set("SHN_DEBUG") || (shn_env_set("SHN_GRAPH_LAPS") && rs.n_reads >= shn_env_u64("SHN_GRAPH_LAPS", 0));
  double tt = tnow();
  auto lapse = [&]() { const double t = tnow(), d = t - tt; tt = t; return d; };
  uint64_t n_kmer_nodes = 0;
  int rc = load_kmer_graph(g, ks, n_kmer_nodes);
  if (rc) return rc;
  lap_line(g.laps, "load_k1mers", lapse(), "rows=%llu", (unsigned long long)ks.n_rows);
  const uint64_t cutoff = n_kmer_nodes * 10, used = std::min<uint64_t>(rs.n_reads, cutoff + 1);      // the read cap
  HostIntakeSlot slot;                                   // (choosing a host form takes the slot -- it counts this call among the host intakes -- until leave() below)
  const IntakePlan plan = choose_intake(rs, g.ctx, K, cutoff, slot);
  const bool on_device = plan.form == IntakeForm::DeviceAttrs || plan.form == IntakeForm::DeviceDedup;
  ScratchLease lease(g.reads, (size_t)used * rs.nm() * (size_t)rs.read_len() / (on_device ? 2 : 1));
  if ((rc = g.reads.load(g.ctx, rs, used, plan))) return rc;
  slot.leave();
  lap_line(g.laps, "load reads", lapse(), "reads=%llu distinct=%zu", (unsigned long long)rs.n_reads, g.reads.n_rd());
  rc = g.run();
  g.release_gpu();
  if (rc) return rc;
  tt = tnow();
  *out = export_components(g);
  lap_line(g.laps, "output_components", lapse(), "%s", "");
  return SHN_OK;
}

// reads: ASCII or codes (enc: SHN_ENC_ASCII or SHN_ENC_CODES, 0..3) with r_off[n_reads+1]; paired: second mate file r2 / r2_off
// with the same count; rc1 / rc2: the strand-doubled view of the packed input, shannon.py:396-424
static ReadSource text_reads(const uint8_t* r1, const uint64_t* r1_off, const uint8_t* r2, const uint64_t* r2_off, uint64_t n_reads, int paired, int enc,
                             const uint8_t* rc1, const uint8_t* rc2) {
  ReadSource rs;
  rs.r1 = r1; rs.r1_off = r1_off; rs.r2 = r2; rs.r2_off = r2_off; rs.n_reads = n_reads; rs.paired = paired; rs.enc = enc; rs.rc1 = rc1; rs.rc2 = rc2;
  return rs;
}

extern "C" int shn_mbgraph_run(shn_ctx* ctx, int K, const uint8_t* rows, uint64_t n_rows, const uint8_t* r1, const uint64_t* r1_off,
                               const uint8_t* r2, const uint64_t* r2_off, uint64_t n_reads, int paired, int enc, const uint8_t* rc1,
                               const uint8_t* rc2, shn_graph** out) {
  ReadSource rs = text_reads(r1, r1_off, r2, r2_off, n_reads, paired, enc, rc1, rc2);
  return mbgraph_run(ctx, K, KmerGraphSource{rows, n_rows, nullptr, 0}, rs, out);
}
// The same with the partition's K-mer graph already contracted on the GPU (see KmerGraphSource).
extern "C" int shn_mbgraph_run_unitigs(shn_ctx* ctx, const shn_unitigs* ug, uint32_t part, const uint8_t* rows, uint64_t n_rows, const uint8_t* r1,
                                       const uint64_t* r1_off, const uint8_t* r2, const uint64_t* r2_off, uint64_t n_reads, int paired, int enc,
                                       const uint8_t* rc1, const uint8_t* rc2, shn_graph** out) {
  if (!ug || part >= ug->n_parts) return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run_unitigs: bad unitigs / partition");
  ReadSource rs = text_reads(r1, r1_off, r2, r2_off, n_reads, paired, enc, rc1, rc2);
  return mbgraph_run(ctx, ug->K, KmerGraphSource{rows, n_rows, ug, part}, rs, out);
}

// The same again with the partition's reads known as rows of the resident input (src_a / src_b / didx, see ReadSource).  The read
// text (r1 / r2) is still what the host side of the stage works on; the device copy of the distinct reads is gathered from the
// resident sets instead of uploaded.
extern "C" int shn_mbgraph_run_resident(shn_ctx* ctx, const shn_unitigs* ug, uint32_t part, const uint8_t* rows, uint64_t n_rows, const shn_reads* src_a,
                                        const shn_reads* src_b, const uint32_t* didx, const uint8_t* r1, const uint64_t* r1_off, const uint8_t* r2,
                                        const uint64_t* r2_off, uint64_t n_reads, int paired, int enc, const uint8_t* rc1, const uint8_t* rc2,
                                        shn_graph** out) {
  if (!ug || part >= ug->n_parts) return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run_resident: bad unitigs / partition");
  ReadSource rs = text_reads(r1, r1_off, r2, r2_off, n_reads, paired, enc, rc1, rc2);
  rs.src_a = src_a; rs.src_b = src_b; rs.didx = didx;
  return mbgraph_run(ctx, ug->K, KmerGraphSource{rows, n_rows, ug, part}, rs, out);
}

// The partition's reads named only by their rows: host_a / host_b = the run's reads as host code matrices (uint8 codes 0-3,
// [n_reads of the set][read length], the same reads as src_a / src_b hold packed on the device), didx as above.  The distinct
// reads are found on the device (shn_reads_dedup) and only their text is decoded on the host, straight from the matrices: no
// per-partition copy of the routed reads exists anywhere.
static int mbgraph_run_rows(shn_ctx* ctx, const shn_unitigs* ug, uint32_t part, const uint8_t* rows, uint64_t n_rows, const shn_reads* src_a,
                            const shn_reads* src_b, const uint8_t* host_a, const uint8_t* host_b, const uint32_t* didx, const uint32_t* d_didx,
                            uint64_t n_reads, int paired, shn_graph** out) {
  if (!ug || part >= ug->n_parts) return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run_rows: bad unitigs / partition");
  if (!ctx || !src_a || !host_a || (n_reads && !didx && !d_didx) || (paired && (!src_b || !host_b)) || !src_a->fixed_len ||
      (paired && src_b->fixed_len != src_a->fixed_len))
    return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run_rows: needs a context, fixed-length resident read sets and their host matrices");
  const bool dbg = shn_env_set("SHN_GRAPH_LAPS") && n_reads >= shn_env_u64("SHN_GRAPH_LAPS", 0);
  const double t0 = dbg ? tnow() : 0.0;
  ReadSource rs;
  rs.src_a = src_a; rs.src_b = src_b; rs.host_a = host_a; rs.host_b = host_b; rs.didx = didx; rs.d_didx = d_didx;
  rs.n_reads = n_reads; rs.paired = paired; rs.enc = SHN_ENC_CODES;
  const int rc = mbgraph_run(ctx, ug->K, KmerGraphSource{rows, n_rows, ug, part}, rs, out);
  if (dbg) fprintf(stderr, "[mbgraph] the call (partition %u), its clean-up included %8.3f s\n", part, tnow() - t0);
  return rc;
}
extern "C" int shn_mbgraph_run_rows(shn_ctx* ctx, const shn_unitigs* ug, uint32_t part, const uint8_t* rows, uint64_t n_rows, const shn_reads* src_a,
                                    const shn_reads* src_b, const uint8_t* host_a, const uint8_t* host_b, const uint32_t* didx, uint64_t n_reads,
                                    int paired, shn_graph** out) {
  return mbgraph_run_rows(ctx, ug, part, rows, n_rows, src_a, src_b, host_a, host_b, didx, nullptr, n_reads, paired, out);
}
// The same with the partition's routed reads named a second time by where they already lie on the device: entries [route_lo,
// route_lo + n_reads) of the routes shn_route_reads left there (didx = the same indices on the host) -- the duplicate search then
// reads them in place instead of uploading the list again (0.5 GB per step at BASELINE configs[2], in 111 pieces).
extern "C" int shn_mbgraph_run_routes(shn_ctx* ctx, const shn_unitigs* ug, uint32_t part, const uint8_t* rows, uint64_t n_rows, const shn_reads* src_a,
                                      const shn_reads* src_b, const uint8_t* host_a, const uint8_t* host_b, const uint32_t* didx, const shn_routes* routes,
                                      uint64_t route_lo, uint64_t n_reads, int paired, shn_graph** out) {
  if (!routes) return shn_fail(SHN_ERR_ARG, "shn_mbgraph_run_routes: routes is NULL");
  const uint32_t* d = nullptr;
  int rc = shn_routes_device_slice(routes, route_lo, n_reads, &d);
  if (rc) return rc;
  return mbgraph_run_rows(ctx, ug, part, rows, n_rows, src_a, src_b, host_a, host_b, didx, d, n_reads, paired, out);
}

// sizes: [n_singles, s_bases, n_comps, n_nodes, n_bases, n_edges, n_paths, n_path_ids, n_info]
extern "C" int shn_graph_sizes(const shn_graph* g, uint64_t* sizes) {
  if (!g || !sizes) return shn_fail(SHN_ERR_ARG, "shn_graph_sizes: NULL argument");
  sizes[0] = g->s_cc.size(); sizes[1] = g->s_bases.size(); sizes[2] = g->comp_node_off.size() - 1; sizes[3] = g->n_cc.size();
  sizes[4] = g->n_bases.size(); sizes[5] = g->e_in.size(); sizes[6] = g->p_off.size() - 1; sizes[7] = g->p_ids.size();
  sizes[8] = g->info.size();
  return SHN_OK;
}

extern "C" int shn_graph_export(const shn_graph* g, uint64_t* s_off, uint8_t* s_bases, double* s_cc, double* s_norm,
                                uint64_t* comp_node_off, uint64_t* comp_edge_off, uint64_t* comp_path_off, uint64_t* n_off,
                                uint8_t* n_bases, double* n_cc, uint8_t* n_cc_int, double* n_norm, int32_t* e_in, int32_t* e_out,
                                int32_t* e_w, double* e_cc, double* e_norm, uint64_t* p_off, int32_t* p_ids, int32_t* info) {
  if (!g) return shn_fail(SHN_ERR_ARG, "shn_graph_export: NULL graph");
#define CP(dst, v) if (dst && !(v).empty()) memcpy(dst, (v).data(), (v).size() * sizeof((v)[0]))
  CP(s_off, g->s_off); CP(s_bases, g->s_bases); CP(s_cc, g->s_cc); CP(s_norm, g->s_norm);
  CP(comp_node_off, g->comp_node_off); CP(comp_edge_off, g->comp_edge_off); CP(comp_path_off, g->comp_path_off);
  CP(n_off, g->n_off); CP(n_bases, g->n_bases); CP(n_cc, g->n_cc); CP(n_cc_int, g->n_cc_int); CP(n_norm, g->n_norm);
  CP(e_in, g->e_in); CP(e_out, g->e_out); CP(e_w, g->e_w); CP(e_cc, g->e_cc); CP(e_norm, g->e_norm);
  CP(p_off, g->p_off); CP(p_ids, g->p_ids); CP(info, g->info);
#undef CP
  return SHN_OK;
}

// The inverse of shn_graph_export: a shn_graph from flattened component tables (sizes[9] as shn_graph_sizes; arrays as
// shn_graph_export, info may be NULL) -- lets the native sparse-flow stage run on tables that did not come from
// shn_mbgraph_run (the reference's own nodes / edges / paths files in the tests).
extern "C" int shn_graph_from_tables(const uint64_t* sizes, const uint64_t* s_off, const uint8_t* s_bases, const double* s_cc, const double* s_norm,
                                     const uint64_t* comp_node_off, const uint64_t* comp_edge_off, const uint64_t* comp_path_off, const uint64_t* n_off,
                                     const uint8_t* n_bases, const double* n_cc, const uint8_t* n_cc_int, const double* n_norm, const int32_t* e_in,
                                     const int32_t* e_out, const int32_t* e_w, const double* e_cc, const double* e_norm, const uint64_t* p_off,
                                     const int32_t* p_ids, shn_graph** out) {
  if (!sizes || !out) return shn_fail(SHN_ERR_ARG, "shn_graph_from_tables: NULL argument");
  shn_graph* g = new shn_graph();
  const uint64_t ns = sizes[0], sb = sizes[1], nc = sizes[2], nn = sizes[3], nb = sizes[4], ne = sizes[5], np = sizes[6], npid = sizes[7];
  g->s_off.assign(s_off, s_off + ns + 1); g->s_bases.assign((const char*)s_bases, sb); g->s_cc.assign(s_cc, s_cc + ns); g->s_norm.assign(s_norm, s_norm + ns);
  g->comp_node_off.assign(comp_node_off, comp_node_off + nc + 1); g->comp_edge_off.assign(comp_edge_off, comp_edge_off + nc + 1);
  g->comp_path_off.assign(comp_path_off, comp_path_off + nc + 1);
  g->n_off.assign(n_off, n_off + nn + 1); g->n_bases.assign((const char*)n_bases, nb); g->n_cc.assign(n_cc, n_cc + nn); g->n_norm.assign(n_norm, n_norm + nn);
  g->n_cc_int.assign(n_cc_int, n_cc_int + nn);
  g->e_in.assign(e_in, e_in + ne); g->e_out.assign(e_out, e_out + ne); g->e_w.assign(e_w, e_w + ne); g->e_cc.assign(e_cc, e_cc + ne); g->e_norm.assign(e_norm, e_norm + ne);
  g->p_off.assign(p_off, p_off + np + 1); g->p_ids.assign(p_ids, p_ids + npid);
  *out = g;
  return SHN_OK;
}
